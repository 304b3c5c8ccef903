/*
 * localdiff_hip.h -- C-ABI of the MI355X (gfx950) local-diffusion sampling hot path.
 *
 * The reference (edshkim98/LocalDiffusion-Hallucination) has no FFI boundary of its own: its hot
 * path sits behind two Python nn.Module surfaces, Unet.forward (ddpm.py:404-451) and
 * GaussianDiffusion.sample / p_sample_loop / ddim_sample / p_sample (ddpm.py:841-1125), whose
 * bodies are stock ATen ops.  This library is what a ctypes binding on the reference side would
 * call instead of those ATen ops; every entry point names the reference lines
 * whose arithmetic it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless marked "host".
 *   - every launch function takes the HIP stream to enqueue on (void*, a hipStream_t) and returns
 *     0 on success or a negative LD_E* code; ld_last_error() gives a thread-local message.
 *   - no allocation and no synchronisation inside launch functions, so they may be captured into a HIP graph
 *     (ld_graph_*).  The library's only process-wide mutable state is what this header documents further down: the
 *     launch-routing table (ld_tuning_set / ld_tuning_get: read by the launch functions, written only by an explicit
 *     call or once from the environment), the launch-routing counters (ld_counter: diagnostics, relaxed atomics) and
 *     the per-thread word of the last launched route (ld_last_route: a diagnostic too), the
 *     per-(kernel, device) LDS-limit cache and an open timing session (ld_timing_*); none of it changes what a launch
 *     computes, only which kernel variant computes it.
 *   - internal activations are NHWC (channels-last) in the storage dtype (LD_F32, LD_BF16 or LD_F16),
 *     accumulation is always fp32 (the 16-bit types run v_mfma_f32_16x16x32_bf16 / _f16 at the same rate; fp16
 *     keeps 10 mantissa bits against bf16's 7, at a range of 6e-8 .. 65504); tensors that cross the reference's API (x_t, cond, mask, model
 *     output) are NCHW fp32 exactly as the reference holds them.
 *   - "t_ptr" arguments are device pointers to the current timestep index (int32).  Kernels read
 *     the step through them so that one captured graph can be replayed for every timestep; pass
 *     NULL to mean row 0 of the table argument.
 */
#ifndef LOCALDIFF_HIP_H
#define LOCALDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LD_OK 0
#define LD_EINVAL (-1)   /* bad argument / unsupported shape */
#define LD_EHIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define LD_ETIMEOUT (-3) /* a deadline passed (ld_comm_init_timeout and the calls on the communicator it made) */

#define LD_F32 0
#define LD_BF16 1
#define LD_F16 2

/* GroupNorm statistics buffers are [B, LD_STAT_STRIPES, groups, 2] fp64 (sum, sum of squares):
 * a producer workgroup adds into stripe (workgroup index % LD_STAT_STRIPES) so that the 256
 * workgroups of one image do not serialise on 16 addresses (measured: 23 us per launch at
 * 256x256 with one stripe); the consumer sums the stripes while building its coefficients. */
#define LD_STAT_STRIPES 16

#define LD_ACT_NONE 0
#define LD_ACT_SILU 1
#define LD_ACT_RELU 2

/* ---- runtime ------------------------------------------------------------------------------ */
const char* ld_last_error(void);
int ld_version(void);
/* host out-params: device name (buf, n), compute units, bytes of global memory */
int ld_device_info(char* name, int name_len, int* compute_units, int64_t* global_mem_bytes);
/* HIP-graph capture of everything enqueued on `stream` between begin and end (no tracing compiler:
 * the host issues the step once, the graph replays it T times). */
int ld_graph_begin(void* stream);
int ld_graph_end(void* stream, void** graph_exec_out);
int ld_graph_launch(void* graph_exec, void* stream);
int ld_graph_destroy(void* graph_exec);
/* hipMemsetAsync(ptr, 0, bytes) on the stream (statistics arenas are zeroed once per forward) */
int ld_memset_zero(void* ptr, size_t bytes, void* stream);
/* hipMemsetAsync(ptr, value & 0xff, bytes): the activation pool's verify mode poisons dead buffers with 0xFF (NaN in every storage type) */
int ld_memset_bytes(void* ptr, int value, size_t bytes, void* stream);
/* event timing on the stream the kernels run on (bench.py's roofline leg) */
/* Per-launch timing session: between begin and end every kernel launched by this library (from the calling
 * process, any stream) carries its own start/stop events; ld_timing_count() = launches so far, ld_timing_end fills
 * ms[i] with launch i's execution time (dispatch begin -> end, what rocprofv3 --kernel-trace reports). */
int ld_timing_begin(int max_launches);
int ld_timing_count(void);
int ld_timing_end(float* ms, int cap, int* count);
/* the same, with the launches' positions on the device clock: start_ms[i] / stop_ms[i] = begin / end of launch i relative
 * to the begin of launch 0 (one clock for every stream: the overlap of launches on different streams can be read off) */
int ld_timing_end_abs(float* start_ms, float* stop_ms, int cap, int* count);
int ld_event_create(void** ev_out);
int ld_event_record(void* ev, void* stream);
int ld_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out); /* synchronises on stop */
int ld_event_destroy(void* ev);
/* make `stream` wait for `ev` (fork/join of independent branches on two streams, e.g. a ResnetBlock's
 * res_conv beside its 3x3 convs; also captured as graph edges) */
int ld_stream_wait_event(void* stream, void* ev);
/* ---- tuning: the launch-routing thresholds of the library, ONE table per process ------------------------------------
 * Every threshold a dispatcher consults (which tile variant, grouped K staging, the persistent C=32 convolution, ...)
 * is an entry of this table: defaults compiled in, an environment override LD_<NAME IN CAPITALS> read ONCE when the
 * table is first used, and explicit control through ld_tuning_set (what localdiffusion_hallucination_amd.tuning.Tuning
 * applies).  Names (defaults): c1_group (1), c1_group_max_px (32768), c1_group_min_ch (4), c1_pair_max_px (2^40),
 * c1_small_min (256), c1_big_min (512: workgroups of 256-pixel tiles from which ld_conv1x1 uses them instead of 128-pixel ones), conv_raw (1), conv_mt4_min_wgs (256), conv_big_min (512), conv_sk (0), conv_sk_max_wgs (256),
 * conv_c32 (0: the persistent LDS-DMA kernel is retired from the default routing, finding 99), conv_c32_min_tiles (2048), gn_frags_per_block (512), fold_split_min (32), attn_split_max_wgs (256), attn_split_min_n
 * (2048; and the two-key-group kernel is only taken when the second group owns a key: n > tile size), lead_args (1: gn_apply /
 * conv1x1 launches that qualify use the kernels with preloaded leading arguments), conv_s32 (3: bit mask of the launches the lean
 * Cout = 32 kernel of conv3x3_s32.hip takes -- 1 single-chunk without prologue, 2 with the GroupNorm prologue, 4 two-chunk),
 * conv_s32_min_tiles (1024: 16 x 16 tiles per launch from which it is used), attn_xcd_map (1: ld_attention's XCD-aware workgroup
 * order), conv_big4_min (256: workgroups of the 64-channel x 16-row tile from which ld_conv3x3 uses it instead of 64 x 8 rows).
 * Values change routing, never
 * results beyond the summation order of a tile variant.  Unknown name: LD_EINVAL.  Not thread-safe against concurrent
 * launches (set it before launching).  The reference has no counterpart (its tuning is cuDNN's). */
int ld_tuning_set(const char* name, long long value);
int ld_tuning_get(const char* name, long long* value_out);
int ld_tuning_count(void);
const char* ld_tuning_name(int index);              /* NULL past the end */
/* Profiler-visible phase markers: nested roctx ranges (host side) around the phases of a sample -- "encoder",
 * "step", "exchange" -- so that a rocprofv3 --marker-trace of sample() is readable.  The reference's only hook is the
 * wall-clock timer around sample() (test.py:392-415).  No-ops when no roctx library can be loaded (LD_NO_ROCTX=1:
 * never try). */
/* Host-side counters of how the dispatchers routed launch calls since the library was loaded (a call made during
 * graph capture counts once, its replays do not): lets a test assert WHICH kernel a shape ran on. */
#define LD_COUNTER_CONV3X3_C32 0      /* ld_conv3x3 calls taken by the persistent LDS-DMA kernel (conv3x3_c32.hip) */
#define LD_COUNTER_CONV3X3_GENERIC 1  /* ... by the register-staged generic kernel (conv3x3.hip) */
#define LD_COUNTER_CONV3X3_S32 2      /* ... by the lean Cout = 32 large-map kernel (conv3x3_s32.hip) */
#define LD_COUNTER_MAX 8
long long ld_counter(int which);
/* The tile variant that the CALLING THREAD's most recent successful ld_conv3x3 / ld_conv1x1 call launched, as a packed
 * word; -1 before the thread's first such launch (a refused call leaves the word as it was).  A diagnostic beside
 * ld_counter: lets a test assert WHICH instantiation a shape ran on instead of inferring it from the thresholds.
 *   LD_ROUTE_CONV3X3: bits 0-3 kernel family (0 generic conv3x3.hip, 1 lean conv3x3_s32.hip, 2 persistent
 *     conv3x3_c32.hip); bits 4-7 MT (16-channel tiles per workgroup); bits 8-11 NW (16-pixel rows per wave: 4 NW rows per
 *     tile); bit 12 RAW (the instantiation without the GroupNorm prologue); bit 13 SK (split-K halves); bit 14 SIDE (the
 *     res_conv side output).  The lean and persistent kernels report their 32-channel x 16-row tile as MT 2, NW 4, and RAW
 *     when the launch carried no GroupNorm prologue.
 *   LD_ROUTE_CONV1X1: bits 0-3 MT; bits 4-7 NW (64 NW pixels per tile); bits 8-11 the epilogue instantiation (LD_EPI_*;
 *     6 = LD_EPI_GN_TAIL with `residual` set); bits 12-15 G (K-chunks staged per barrier pair: 1, 2 or 4); bits 16-17 the
 *     argument passing (0 the argument block, 1 preloaded sources / weights "klead", 2 preloaded tail operand "tlead"). */
#define LD_ROUTE_CONV3X3 0
#define LD_ROUTE_CONV1X1 1
#define LD_ROUTE_MAX 2
long long ld_last_route(int op);
int ld_range_push(const char* name /* host string */);
int ld_range_pop(void);

/* ---- one input of a convolution, with an optional normalise-on-load prologue --------------- */
/* Replaces the separate GroupNorm / FiLM / SiLU / ReLU / concat / nearest-upsample passes of
 * Block.forward (ddpm.py:177-186), ResnetBlock.forward (:200-212), Upsample (:114-118),
 * torch.cat (:435,439,442,448) and BasicBlock (unet_model.py:19-26): the consumer convolution
 * applies  y = act(x * a[b,c] + s[b,c])  while staging its input tile, where a,s come from the
 * producer's GroupNorm statistics (sum, sum of squares per (batch, group), fp64), gamma/beta and
 * the FiLM (scale+1, shift) row of this timestep. */
typedef struct ld_src {
  const void* data;        /* NHWC [B, Hs, Ws, C], storage dtype */
  int32_t C;               /* channels (multiple of 32) */
  int32_t pix_stride;      /* elements between consecutive pixels; 0 = C (dense). Lets a conv read a
                              channel slice, e.g. q = channels [0,hidden) of a qkv tensor */
  int32_t upsample;        /* 1: source is [B, H/2, W/2, C], read with nearest x2 */
  const double* gn_stats;  /* [B, LD_STAT_STRIPES, groups, 2] or NULL = no prologue */
  const float* gn_gamma;   /* [C] */
  const float* gn_beta;    /* [C] */
  int32_t gn_groups;
  int32_t act;             /* LD_ACT_* applied after the affine */
  const float* film;       /* [rows, 2*C] (scale | shift) or NULL */
  int32_t film_tstride;    /* floats between timestep rows (0 if per-batch rows only) */
  int32_t film_bstride;    /* floats between batch rows (0 if shared by the batch) */
} ld_src;

/* ---- 3x3 convolution, pad 1, implicit GEMM on MFMA ----------------------------------------- */
/* nn.Conv2d(k=3,p=1): Block.proj (ddpm.py:173), Upsample conv (:117), stage convs (:372,:391),
 * BasicBlock convs (unet_model.py:20,24,30).  Epilogue adds bias and (optionally) accumulates the
 * GroupNorm statistics of the result for the next layer (ddpm.py:174 / unet_model.py:21,25,31). */
typedef struct ld_conv3x3_args {
  ld_src src[2];           /* channel-concatenated inputs (torch.cat order) */
  int32_t nsrc;
  const void* weight;      /* packed by ld_pack_conv_weight, storage dtype */
  const float* bias;       /* [Cout] fp32 */
  void* out;               /* NHWC [B,H,W,Cout] */
  double* out_stats;       /* [B, LD_STAT_STRIPES, out_groups, 2] accumulated (caller zeroes) or NULL */
  int32_t out_groups;      /* Cout / out_groups (channels per group) must divide 32: 1, 2, 4, 8, 16 or 32; else LD_EINVAL */
  int32_t B, H, W, Cout;   /* Cout multiple of 32 */
  const int32_t* t_ptr;
  int32_t dtype;
  const void* addend;      /* optional NHWC [B,H,W,Cout] tensor (storage dtype) added to conv + bias BEFORE the     */
                           /* statistics: the step-invariant half of a convolution over a concatenation whose     */
                           /* second operand does not change between reverse steps (conv_fusion, ddpm.py:434-436) */
  int32_t weight_terms;    /* 0 / 1: `weight` from ld_pack_conv_weight; 2: two-term weights from                    */
                           /* ld_pack_conv_weight_terms(..., 2) (16-bit storage): x*hi + x*lo, weights exact to 2^-17 */
  const void* side_weight; /* optional second output of the launch (16-bit storage, raw sources): a 1x1 convolution of the  */
  const float* side_bias;  /* SAME concatenated input -- the ResnetBlock's res_conv (ddpm.py:198, 212) beside its block1     */
  void* side_out;          /* convolution.  side_weight [Cout, Cin] packed by ld_pack_conv_weight(ksize 1), side_bias [Cout],  */
                           /* side_out NHWC [B,H,W,Cout] = W_side x + side_bias (no statistics).  NULL = none.              */
} ld_conv3x3_args;
int ld_conv3x3(const ld_conv3x3_args* args, void* stream);
/* The kernel ld_conv3x3 would launch for *args under the current routing table, as an LD_ROUTE_CONV3X3 word,
   without launching anything; a negative LD_E* code where ld_conv3x3 would refuse the arguments (ld_last_error
   set as ld_conv3x3 sets it).  Pointers are tested for null only.  Needs no GPU.  Does not change ld_last_route.
   It IS the decision ld_conv3x3 launches by, not a copy of it (a library built with --debug-variants can override the
   decision from the environment in ways this query does not predict). */
long long ld_conv3x3_route(const ld_conv3x3_args* args);

/* ---- 1x1 convolution (GEMM over channels) -------------------------------------------------- */
#define LD_EPI_PLAIN 0      /* out = W x + b                                                    */
#define LD_EPI_QKV_LINEAR 1 /* LinearAttention.to_qkv (ddpm.py:239-245): first `hidden` outputs   */
                            /* (q) get softmax over each head's 32 channels times dim_head^-0.5  */
#define LD_EPI_QKV_FULL 2   /* Attention.to_qkv (ddpm.py:276) with attend.py:98's scale folded   */
                            /* into q                                                           */
#define LD_EPI_RMS_RES 3    /* to_out conv + RMSNorm + residual (ddpm.py:229-232,251,425,444)    */
#define LD_EPI_RES 4        /* to_out conv + residual (ddpm.py:269,282,425,431)                  */
#define LD_EPI_GN_TAIL 5    /* ResnetBlock tail fused into its res_conv (ddpm.py:198,210-212);    */
                            /* `residual`, if given, is added too (step-invariant half of res_conv) */
                            /* out = res_conv(x) + act(GroupNorm(gn_tail))  -- gn_tail is block2's */
                            /* raw conv output with its statistics                               */
typedef struct ld_conv1x1_args {
  ld_src src[2];
  int32_t nsrc;
  int32_t unshuffle;       /* 1: Downsample (ddpm.py:120-124): src[0] is [B,2H,2W,C], K = 4C in  */
                           /*    (p1,p2,c) order (weights repacked accordingly)                  */
  int32_t rms_in;          /* 1: RMSNorm on the input (ddpm.py:131-132): columns scaled by        */
                           /*    1/max(||x_p||,1e-12); g*sqrt(C) is folded into `weight`          */
  const void* weight;
  int64_t weight_bstride;  /* bytes between per-batch weight sets (linear attention) or 0        */
  const float* bias;       /* [Cout] or NULL */
  int32_t epilogue;        /* LD_EPI_* */
  int32_t hidden;          /* heads*dim_head for the QKV epilogues */
  float q_scale;           /* dim_head^-0.5 */
  const float* g2;         /* [Cout] g*sqrt(Cout) for LD_EPI_RMS_RES */
  const void* residual;    /* NHWC [B,H,W,Cout] for *_RES */
  ld_src gn_tail;          /* LD_EPI_GN_TAIL: NHWC [B,H,W,Cout] + GroupNorm prologue fields (no FiLM) */
  void* out;
  uint32_t* kmax_out;      /* LD_EPI_QKV_LINEAR only, optional: [B, LD_STAT_STRIPES, hidden] order-encoded running max
                              of the k channels over pixels (integer atomicMax; caller zeroes) -- see ld_linattn_kmax */
  int32_t B, H, W, Cout;
  int32_t dtype;
  int32_t weight_terms;    /* as in ld_conv3x3_args (not with rms_in or per-batch weights) */
} ld_conv1x1_args;
int ld_conv1x1(const ld_conv1x1_args* args, void* stream);

/* Repack an OIHW fp32 convolution weight (device) into the MFMA fragment order the kernels read.
 * ksize 1 or 3.  `scale_in` (optional, [Cin]) multiplies input channel c (RMSNorm g*sqrt(C)).
 * unshuffle=1 reorders K from (c,p1,p2) to (p1,p2,c).  out must hold Cout*Cin*k*k elements. */
int ld_pack_conv_weight(const float* w_oihw, const float* scale_in, void* out, int cout, int cin,
                        int ksize, int unshuffle, int dtype, void* stream);
/* terms = 2 (16-bit storage): two-term weights W = hi + lo, hi = round(W), lo = round(W - hi); out holds twice the
 * elements, every K-chunk of hi followed by its chunk of lo.  Consumed by ld_conv3x3 / ld_conv1x1 with
 * weight_terms = 2 at twice the matrix work: rounding the WEIGHTS to 16 bits is what separates a 16-bit sampling chain
 * from the reference's fp32 weights (the same perturbation at every reverse step; activation roundings average out). */
int ld_pack_conv_weight_terms(const float* w_oihw, const float* scale_in, void* out, int cout, int cin,
                              int ksize, int unshuffle, int dtype, int terms, void* stream);

/* ---- small-Cin direct convolution from an NCHW fp32 image --------------------------------- */
/* init_conv 7x7 (ddpm.py:319,413) and the first BasicBlock convs (unet_model.py:20,30) whose
 * Cin is 1 or 3.  Cout must be 32.  Output NHWC storage dtype (+ optional GN statistics). */
int ld_conv_image(const float* x_nchw, const float* w_oihw, const float* bias, void* out,
                  double* out_stats, int out_groups, int B, int Cin, int H, int W, int ksize,
                  int dtype, void* stream);

/* init_conv 7x7 (ddpm.py:319,413) for 16-bit storage as an implicit GEMM on MFMA: x NCHW fp32 [B,Cin<=3,H,W] ->
 * out NHWC bf16 / fp16 [B,H,W,32].  Image and weights are split into bf16 hi+lo parts (three MFMA products, fp32
 * accumulate), so the result equals the fp32-FMA kernel of ld_conv_image up to the rounding of the stored bf16.
 * w_packed: ld_stem_packed_bytes() bytes written once per model by ld_pack_stem_weight from the OIHW fp32 weight. */
size_t ld_stem_packed_bytes(void);
int ld_pack_stem_weight(const float* w_oihw /*[32,Cin,7,7]*/, void* out_packed, int Cin, void* stream);
int ld_conv_stem(const float* x, const void* w_packed, const float* bias, void* out, int B, int Cin, int H, int W,
                 int dtype /* LD_BF16 or LD_F16: type of the stored output */, void* stream);
/* ld_step_begin_film's arguments (below) as a struct, and ld_conv_stem with that head-of-step work folded into the SAME
 * launch: a few extra workgroups zero the arenas, move the step counter and copy the timestep's FiLM row beside the
 * convolution, which reads none of them -- init_conv is the first operation of Unet.forward (ddpm.py:413) and no
 * launch before the third of an evaluation consumes statistics or FiLM, so an evaluation loses its first launch. */
typedef struct ld_step_begin_args {
  void* zero_a; size_t bytes_a; void* zero_b; size_t bytes_b;
  int32_t* t_ptr; int delta; int32_t* idx_ptr; const int32_t* t_table;
  const float* film_rows; int row_floats; float* film_cur;
} ld_step_begin_args;
int ld_conv_stem_begin(const float* x, const void* w_packed, const float* bias, void* out, int B, int Cin, int H, int W,
                       int dtype, const ld_step_begin_args* begin, void* stream);


/* ---- GroupNorm apply (+FiLM) + activation + residual, optional second normalised input ----- */
/* ResnetBlock tail  h = SiLU(GN(conv2)) + res(x)  (ddpm.py:210-212) and BasicBlock tail
 * ReLU(GN(conv2) + GN(conv_id)) followed by MaxPool2d(2) (unet_model.py:38-51,120,123,129). */
typedef struct ld_gn_apply_args {
  ld_src a;                /* first input, prologue required */
  ld_src b;                /* optional second input (data NULL = none); gn_stats NULL = raw add */
  int32_t final_act;       /* LD_ACT_* after the sum */
  int32_t pool;            /* 1: 2x2 max-pool the result (out is [B,H/2,W/2,C]) */
  void* out;
  int32_t B, H, W;         /* input spatial size */
  const int32_t* t_ptr;
  int32_t dtype;
} ld_gn_apply_args;
int ld_gn_apply(const ld_gn_apply_args* args, void* stream);

/* ---- attention ---------------------------------------------------------------------------- */
/* Linear attention core (ddpm.py:243,247,249) on a qkv tensor [B, n, 3*hidden] whose q part was
 * already soft-maxed by ld_conv1x1(LD_EPI_QKV_LINEAR):
 *   1. ld_linattn_kmax:  kmax[b, c] = max_n k[b, n, c] as an order-preserving uint32 code, combined with
 *                        integer atomicMax into a zeroed [B, LD_STAT_STRIPES, hidden] buffer (softmax over n; the
 *                        consumer takes the max over the stripes).
 *                        The product path gets the same buffer for free from ld_conv1x1's kmax_out.
 *   2. ld_linattn_ctx:   partial  ctx[d,e] = sum_n exp(k-max) v,  Z[d] = sum_n exp(k-max) per pixel chunk
 *   3. ld_linattn_ctx_reduce: ctxn[b,h,d,e] = sum_chunks ctx / sum_chunks Z[d]   [B,heads,32,32]
 *   4. ld_linattn_fold:  M_b = W_out . ctxn^T  packed as a per-batch 1x1 weight, so that
 *                        to_out(ctx^T q) becomes ONE 1x1 convolution over q (ld_conv1x1). */
int ld_linattn_kmax(const void* qkv, uint32_t* kmax_enc, int B, int n, int heads, int dim_head,
                    int dtype, void* stream);
int ld_linattn_ctx(const void* qkv, const uint32_t* kmax_enc, float* ctx_part,
                   int B, int n, int heads, int dim_head, int nchunks, int dtype, void* stream);
int ld_linattn_ctx_reduce(const float* ctx_part, int nchunks, float* ctxn, int B, int heads,
                          int dim_head, void* stream);
/* perm=0: standard k=1 packing (consumed by ld_conv1x1); perm=1 (bf16 / fp16): chained-MFMA operand order
 * consumed by ld_linattn_out. */
int ld_linattn_fold(const float* ctxn, const float* w_out /*[C,hidden] fp32*/,
                    void* w_packed /*[B] packed C x hidden*/, int B, int C, int heads, int dim_head,
                    int perm, int dtype, void* stream);
/* Steps 3 + 4 in one launch (grid heads x B x 4): chunk partials -> 8 rows of the normalised context (kept in
 * LDS) -> the matching 8 columns of the packed M_b.  Same arithmetic and output layout as the two calls above. */
int ld_linattn_ctxfold(const float* ctx_part, int nchunks, const float* w_out /*[C,hidden] fp32*/,
                       void* w_packed /*[B] packed C x hidden*/, int B, int C, int heads, int dim_head,
                       int perm, int dtype, void* stream);
/* Fused 16-bit (bf16 / fp16) path: q, k, v never reach HBM (both kernels recompute their slice of to_qkv from x).
 *   ld_linattn_kvctx: x [B,n,C] -> ctx partials (same layout/consumers as ld_linattn_ctx), with the
 *        RMSNorm (ddpm.py:237), the k/v rows of to_qkv (:239) and softmax_n(k) (:243) inside;
 *        wkv_packed = per head the 64 rows (k_h | v_h) of to_qkv, packed k=1 with g*sqrt(C) folded.
 *        kshift (optional, [heads*32] fp32, heads == 4): an upper bound m_d >= max_n k[d] per k channel.
 *        softmax over n is shift-invariant, so exp(k - m_d) / sum_n exp(k - m_d) equals the reference's
 *        exp(k - max) form; with it the kernel makes ONE sweep over x instead of two.  The RMS-normalised
 *        input has unit 2-norm per pixel, hence |k_d| <= ||W_k[d,:] * g * sqrt(C)||_2 (Cauchy-Schwarz): the
 *        host passes that norm, and passes NULL (exact two-sweep maximum) when it exceeds 40, where
 *        exp(k - m_d) could underflow.
 *   ld_linattn_out:   x -> out = RMSNorm(to_out(ctx^T softmax_d(q)*scale)) + x  (:242,245,249,251,425);
 *        wq_packed = the 128 q rows packed the same way, mfold from ld_linattn_fold / _ctxfold (perm=1);
 *        qshift (optional, [4] fp32): per head an upper bound of q over its 32 channels (max_d of the same
 *        Cauchy-Schwarz norm, <= 40), used as the softmax_d shift instead of the per-pixel maximum.
 *        ld_linattn_out / ld_linattn_out_terms are BUILT FOR hidden = 128 (four heads of 32) and take no head count:
 *        they read 128 rows of wq_packed, C x 128 elements of mfold per batch and four floats of qshift whatever the
 *        caller packed, and CANNOT CHECK it.  A caller with another head count must take the unfused route
 *        (ld_conv1x1 LD_EPI_QKV_LINEAR, ld_linattn_ctx, ld_linattn_ctxfold, ld_conv1x1 LD_EPI_RMS_RES), as Unet does.
 *        ld_linattn_kvctx takes any head count in its two-sweep, one-term form (a workgroup per head); kshift and
 *        weight_terms = 2 need heads == 4 and are refused (-1, nothing written) otherwise. */
int ld_linattn_kvctx(const void* x, const void* wkv_packed, const float* kshift, float* ctx_part, int B,
                     int n, int C, int heads, int dim_head, int nchunks, int dtype, void* stream);
int ld_linattn_out(const void* x, const void* wq_packed, const float* qshift, const void* mfold,
                   const float* bias, const float* g2, void* out, int B, int n, int C, float q_scale,
                   int dtype, void* stream);
/* Two-term weights (ld_pack_conv_weight_terms(..., 2) of the same rows, with the RMSNorm scale) for the fused linear
 * attention of the full- and half-resolution blocks (C = 32 / 64, heads = 4): W_kv / W_q enter the matrix pipe as hi + lo.
 * weight_terms = 1 is ld_linattn_kvctx / ld_linattn_out. */
int ld_linattn_kvctx_terms(const void* x, const void* wkv_packed, const float* kshift, float* ctx_part, int B, int n, int C,
                           int heads, int dim_head, int nchunks, int dtype, int weight_terms, void* stream);
int ld_linattn_out_terms(const void* x, const void* wq_packed, const float* qshift, const void* mfold, const float* bias,
                         const float* g2, void* out, int B, int n, int C, float q_scale, int dtype, int weight_terms,
                         void* stream);
size_t ld_linattn_ctx_part_floats(int B, int heads, int dim_head, int nchunks);

/* Full softmax attention (attend.py:84-113) on qkv [B, n, 3*hidden] with q pre-scaled;
 * out [B, n, hidden].  Flash-style (the n x n similarity matrix is never materialised). */
int ld_attention(const void* qkv, void* out, int B, int n, int heads, int dim_head, int dtype,
                 void* stream);

/* ---- timestep embedding (ddpm.py:136-149, 339-344, 191-206) -------------------------------- */
/* temb[i] = Linear(GELU(Linear(sincos(times[i]))))  for i < n;  freqs [dim/2] fp32 (host-made). */
int ld_time_mlp(const int32_t* times, int n, const float* freqs, int dim, const float* w1,
                const float* b1, const float* w2, const float* b2, int time_dim, float* temb,
                void* stream);
/* The same with RandomOrLearnedSinusoidalPosEmb in front (ddpm.py:151-165; learned_sinusoidal_cond / random_fourier_features):
 * emb = [t | sin(2 pi w_k t) | cos(2 pi w_k t)] with the module's `weights` [learned_dim / 2]; w1 is [time_dim, learned_dim + 1]. */
int ld_time_mlp_fourier(const int32_t* times, int n, const float* weights, int learned_dim, const float* w1,
                        const float* b1, const float* w2, const float* b2, int time_dim, float* temb, void* stream);
/* film[i] = Linear(SiLU(temb[i]))  -> [n, 2*C] */
int ld_film(const float* temb, int n, int time_dim, const float* w, const float* b, int two_c,
            float* film, void* stream);

/* ---- final 1x1 conv to the image (ddpm.py:398,451): NHWC storage -> NCHW fp32 -------------- */
int ld_final_conv(const void* x, const float* w /*[Cout,Cin]*/, const float* b, float* out_nchw,
                  int B, int H, int W, int Cin, int Cout, int dtype, void* stream);

/* ld_final_conv + ld_ddpm_step (+ ld_randn for the step's noise, stream index `noise_stream`) of the same pixels
 * in ONE launch: model_out = final_conv(x) is still written (fp32 NCHW), x_t is updated in place to x_{t-1}
 * (ddpm.py:451, 775-776, 659-666, 853-858).  Bitwise the same result as the three separate calls. */
int ld_final_step(const void* x, const float* w, const float* b, float* model_out, float* x_t, float* x0_out,
                  const float* sched, const int32_t* t_ptr, float lo, float hi, int objective, uint64_t seed,
                  int64_t noise_stream, int B, int H, int W, int Cin, int Cout, int dtype, void* stream);


/* ld_final_step for a sub-batch inside a replayed HIP graph: the noise stream index is
 * noise_base + noise_tmul * (*t_ptr) (the sampler's draw counter as a function of the device step counter) and
 * the sub-batch's elements are [noise_first, noise_first + B*Cout*H*W) of that stream's sequence.
 * keep_mask (optional, [B, H*W]): ld_mask_out folded in -- where keep_mask < 1 the prediction is replaced by `lo`
 * before the update (the OOD branch with mask_x, ddpm.py:693-696). */
int ld_final_step_at(const void* x, const float* w, const float* b, float* model_out, float* x_t, float* x0_out,
                     const float* sched, const int32_t* t_ptr, float lo, float hi, int objective, uint64_t seed,
                     int64_t noise_base, int64_t noise_tmul, int64_t noise_first, const float* keep_mask,
                     int B, int H, int W, int Cin, int Cout, int dtype, void* stream);

/* ---- reverse-process pointwise kernels (NCHW fp32) ---------------------------------------- */
#define LD_OBJ_X0 0
#define LD_OBJ_NOISE 1
#define LD_OBJ_V 2
/* schedule table row layout (floats): see LD_SCHED_* ; built by the host from the fp32 buffers */
#define LD_SCHED_COLS 8
#define LD_SCHED_COEF1 0      /* posterior_mean_coef1                (ddpm.py:592) */
#define LD_SCHED_COEF2 1      /* posterior_mean_coef2                (ddpm.py:593) */
#define LD_SCHED_SIGMA 2      /* exp(0.5*posterior_log_variance_clipped) (ddpm.py:591,853) */
#define LD_SCHED_SQRT_RECIP 3 /* sqrt(1/abar)                        (ddpm.py:578) */
#define LD_SCHED_SQRT_RECIPM1 4 /* sqrt(1/abar-1)                    (ddpm.py:579) */
#define LD_SCHED_SQRT_AB 5    /* sqrt(abar)                          (ddpm.py:575) */
#define LD_SCHED_SQRT_1MAB 6  /* sqrt(1-abar)                        (ddpm.py:576) */
#define LD_SCHED_ABAR 7       /* abar                                (ddpm.py:570) */

/* portable counter-based normals (rng.py): stream = stream_base + stream_tmul * (*t_ptr) */
int ld_randn(float* out, int64_t n, uint64_t seed, int64_t stream_base, int64_t stream_tmul,
             const int32_t* t_ptr, void* stream);
/* the slice [first, first + n) of that stream's sequence: sub-batches of one draw generated separately */
int ld_randn_at(float* out, int64_t n, int64_t first, uint64_t seed, int64_t stream_base, int64_t stream_tmul,
                const int32_t* t_ptr, void* stream);
/* *t_ptr += delta  (graph-replayable step counter) */
int ld_step_add(int32_t* t_ptr, int delta, void* stream);
/* head of one denoiser evaluation in ONE launch: zero up to two arenas (GroupNorm statistics, k-max codes; 16-byte
 * aligned and sized; either may be NULL / 0) and move the device step counter BEFORE any kernel of the evaluation
 * reads it: *t_ptr += delta (ancestral loop), or -- when idx_ptr and t_table are given (strided DDIM loop,
 * ddpm.py:984-986) -- *idx_ptr += 1; *t_ptr = t_table[*idx_ptr].  Replaces two hipMemsetAsync nodes + ld_step_add
 * at the head / tail of every replayed step. */
int ld_step_begin(void* zero_a, size_t bytes_a, void* zero_b, size_t bytes_b, int32_t* t_ptr, int delta,
                  int32_t* idx_ptr, const int32_t* t_table, void* stream);
/* the same + the step's FiLM row: film_cur[0 .. row_floats) = film_rows[t_new * row_floats ...] with t_new the counter's
 * value AFTER the move (t_ptr required; delta may be 0) -- the (scale, shift) vectors of every ResnetBlock for this
 * timestep (ddpm.py:191-206 evaluated for all t at setup, ld_film) land at a fixed address, so the launches that apply
 * FiLM need no dependent load of the step counter.  row_floats % 4 == 0, 16-byte aligned rows. */
int ld_step_begin_film(void* zero_a, size_t bytes_a, void* zero_b, size_t bytes_b, int32_t* t_ptr, int delta,
                       int32_t* idx_ptr, const int32_t* t_table, const float* film_rows, int row_floats,
                       float* film_cur, void* stream);

/* p_sample, single branch (ddpm.py:631-666, 739-761, 817-838, 857-858):
 *   x0 = clamp(to_x0(model_out)), x_prev = c1*x0 + c2*x_t + (t>0 ? sigma*z : 0).
 * x0_out may be NULL.  `noise` may be NULL: then no draw is added, in either mode (round 6: table mode used to dereference it
 * at t > 0).  Table mode (`t_ptr` non-NULL) adds sigma*z iff *t_ptr > 0 and `noise` is non-NULL.  Row mode (`t_ptr` NULL:
 * `sched` points at the step's own row, the kernel does not know t) adds it iff `noise` is non-NULL -- the CALLER carries
 * the reference's `t > 0` test (ddpm.py:857): pass NULL at t == 0, or the last step gets noise the reference does not add. */
int ld_ddpm_step(const float* x_t, const float* model_out, const float* noise, float* x_prev,
                 float* x0_out, const float* sched, const int32_t* t_ptr, float lo, float hi,
                 int objective, int64_t n, void* stream);
/* DDIM update (ddpm.py:1046-1068): x0 = clamp(to_x0(model_out)); eps re-derived from x0;
 * x_next = x0*sqrt(abar_next) + c*eps + sigma*z.  Scalars are host-computed per pair.
 * last=1 writes x0 (time_next < 0, :1053-1056). */
int ld_ddim_step(const float* x_t, const float* model_out, const float* noise, float* x_next,
                 float sqrt_recip, float sqrt_recipm1, float sqrt_ab, float sqrt_1mab,
                 float sqrt_abar_next, float c, float sigma, float lo, float hi, int objective,
                 int last, int64_t n, void* stream);
/* ld_ddim_step with the pair's scalars in a device table [pairs, 8] = {sqrt_recip, sqrt_recipm1, sqrt_ab, sqrt_1mab,
 * sqrt_abar_next, c, sigma, last} and the row selected by *idx_ptr: the form a replayed HIP graph needs. */
int ld_ddim_step_at(const float* x_t, const float* model_out, const float* noise, float* x_next,
                    const float* pair_table, const int32_t* idx_ptr, float lo, float hi, int objective, int64_t n,
                    void* stream);
/* branch conditioning (ddpm.py:672-690): binary=(mask>=1); cond_out=cond*binary;
 * cond_in=cond*clip(1-binary, lo_clip, 1).  mask [B,1,H,W], cond [B,C,H,W]. */
int ld_branch_conditions(const float* cond, const float* mask, float* cond_out, float* cond_in,
                         float lo_clip, int B, int C, int HW, void* stream);
/* mask_x on the OOD-branch prediction (ddpm.py:700-703): where(binary==0, min_val, out*binary) */
int ld_mask_out(float* model_out, const float* mask, float min_val, int B, int C, int HW,
                void* stream);
/* DDPM fusion step recomposition (ddpm.py:775-776, 784-804) from per-branch x_t and per-branch
 * x0 predictions (clamped here):  x0 = clamp(clamp(x0_in)*(1-m) + clamp(x0_out));
 *   x = where(x_out*m == 0, x_in*(1-m), x_out*m) */
int ld_fuse_ddpm(const float* x_out, const float* x_in, const float* x0_out, const float* x0_in,
                 const float* mask, float* x, float* x0, float lo, float hi, int B, int C, int HW,
                 void* stream);
/* K-mask generalisation of the two calls above (the reference has K = 2).  masks [B,K,HW]; branch 0
 * is the OOD-style branch, branches 1..K-1 IND-style:
 *   cond_k[0] = cond*(m_0>=1),  cond_k[k] = cond*clip((m_k>=1), lo_clip, 1)            -> cond_k [K,B,C,HW]
 *   x0 = clamp(sum_{k>=1} clamp(x0_k)*(m_k>=1) + clamp(x0_0)),  x = first non-zero of x_k*(m_k>=1), k = 0..K-1
 * x_rest / x0_rest hold branches 1..K-1 contiguously ([K-1,B,C,HW]); branch 0 has its own pointers (its state and
 * prediction may live outside the denoiser's batch, ddpm.py:704-708).  With K = 2 and m_1 = 1-(m_0>=1) the results
 * are bitwise those of ld_branch_conditions / ld_fuse_ddpm. */
int ld_branch_conditions_k(const float* cond, const float* masks, float* cond_k, float lo_clip, int B, int C, int K,
                           int HW, void* stream);
int ld_fuse_ddpm_k(const float* x_first, const float* x_rest, const float* x0_first, const float* x0_rest,
                   const float* masks, float* x, float* x0, float lo, float hi, int B, int C, int K, int HW,
                   void* stream);
/* posterior step from an already-formed x0 (fusion step, ddpm.py:809 + :858) */
int ld_posterior_step(const float* x_t, const float* x0, const float* noise, float* x_prev,
                      const float* sched, const int32_t* t_ptr, int64_t n, void* stream);
/* DDIM fusion (ddpm.py:1025-1041): x0 = clamp(where(x0o==0, x0i, x0o)); eps = where(eo*m==0,
 * ei*(1-m), eo*m) with e* re-derived from the clamped per-branch x0;  x_next as ld_ddim_step. */
int ld_fuse_ddim(const float* x_out, const float* x_in, const float* x0_out, const float* x0_in,
                 const float* mask, const float* noise, float* x_next, float sqrt_recip,
                 float sqrt_recipm1, float sqrt_abar_next, float c, float sigma, float lo,
                 float hi, int B, int C, int HW, void* stream);
/* K-branch form of ld_fuse_ddim (the reference has K = 2): masks [B,K,HW], branch 0 OOD-style with its
 * own pointers, branches 1..K-1 in x_rest / x0_rest ([K-1,B,C,HW]).  Per element, with a_k = clamp(x0_k) and
 * e_k = (sqrt_recip x_k - a_k) / sqrt_recipm1:
 *   x0  = clamp(a_0 if a_0 != 0 else a_j),  j = the first k >= 1 with m_k >= 1, K-1 if there is none
 *   eps = first non-zero of e_k*(m_k>=1), k = 0..K-1 (the last one if all are zero)
 * With K = 2 and m_1 = 1-(m_0>=1) the result is bitwise that of ld_fuse_ddim (ddpm.py:1025-1041). */
int ld_fuse_ddim_k(const float* x_first, const float* x_rest, const float* x0_first, const float* x0_rest,
                   const float* masks, const float* noise, float* x_next, float sqrt_recip, float sqrt_recipm1,
                   float sqrt_abar_next, float c, float sigma, float lo, float hi, int B, int C, int K, int HW,
                   void* stream);
/* q_sample (ddpm.py:1148-1154) for the use_gt start (:937-944) */
int ld_q_sample(const float* x0, const float* noise, float* out, float sqrt_ab, float sqrt_1mab,
                int64_t n, void* stream);
/* ---- training-side forward (forward half): GaussianDiffusion.forward / p_losses, ddpm.py:1147-1214 -----
 * q_sample with one timestep per sample: out_b = sqrt_ab[t_b] x0_b + sqrt_1mab[t_b] noise_b  (t: int32 [B] on the
 * device, sqrt_ab / sqrt_1mab: the fp32 schedule buffers [T] on the device). */
int ld_q_sample_t(const float* x0, const float* noise, float* out, const int* t, const float* sqrt_ab,
                  const float* sqrt_1mab, int B, int64_t elems_per_sample, void* stream);
/* per-sample loss (:1186-1201): loss_out[b] = loss_weight[t_b] * mean_{c,h,w} (model_out - target)^2, target = noise
 * (LD_OBJ_NOISE) | x_start (LD_OBJ_X0) | sqrt_ab[t_b] noise - sqrt_1mab[t_b] x_start (LD_OBJ_V, predict_v :643-647).
 * fp32 NCHW operands, fp64 accumulation in a fixed order; the batch mean (:1201) is the caller's. */
int ld_p_losses(const float* model_out, const float* x_start, const float* noise, const int* t, const float* sqrt_ab,
                const float* sqrt_1mab, const float* loss_weight, float* loss_out, int B, int64_t elems_per_sample,
                int objective, void* stream);
/* recomposition of K gathered local patches by their masks (north-star multi-GPU path,
 * SURVEY.md 8e): out[b] = sum_k patches[b,k]*m_k  with m_k = (masks[k] >= 1) */
int ld_recompose(const float* patches /*[B,K,C,HW]*/, const float* masks /*[K,HW]*/, float* out,
                 int B, int K, int C, int HW, void* stream);

/* ---- segmentation U-Net: the OOD-mask producer in front of sample() --------------------------------------------------
 * UNet(n_channels, 1, bilinear=False) of unet_model.py:140-243, which test.py:214-221, 284-289 runs on the shifted
 * conditioning image (mask = sigmoid(logits) > 0.5).  Every DoubleConv convolution (conv3x3, no bias) carries BatchNorm2d
 * (eval) + ReLU as an fp32 epilogue on the fp32 accumulator: out = relu(acc * scale[c] + shift[c]), scale = gamma /
 * sqrt(running_var + eps), shift = beta - running_mean * scale (host-made; the weights are not scaled).  Activations are
 * NHWC in the storage dtype, weights fp32.  The diffusion path's kernels above are not involved. */
#define LD_SEG_SRC_PLAIN 0    /* src0 [B, H, W, C0]                                                                  */
#define LD_SEG_SRC_POOL 1     /* src0 [B, 2H, 2W, C0] read through a 2x2 max-pool (Down, unet_model.py:170-180)       */
#define LD_SEG_SRC_CAT_D2S 2  /* cat([src0 [B, H, W, C0], depth_to_space(src1 [B, H/2, W/2, 4*C1])]) (Up, :197-206):  */
                              /* channel c of pixel (y, x) of the second part is element ((y&1)*2 + (x&1))*C1 + c of    */
                              /* low-res pixel (y>>1, x>>1) -- the layout ld_seg_conv(ksize 1) writes for a ConvTranspose2d */
typedef struct ld_seg_conv_args {
  const void* src0;        /* see LD_SEG_SRC_* */
  const void* src1;        /* LD_SEG_SRC_CAT_D2S only */
  int32_t C0, C1;          /* channels of src0 / of the depth-to-space part (multiples of 32; C1 = 0 unless CAT_D2S) */
  int32_t mode;            /* LD_SEG_SRC_* */
  int32_t ksize;           /* 3 (pad 1), or 1 with a plain source: ConvTranspose2d(2, 2) as a GEMM to 4*Cout channels */
  const float* weight;     /* fp32 [ksize*ksize][C0 + C1][Cout] from ld_seg_pack_weight / ld_seg_pack_convt */
  const float* scale;      /* [Cout] or NULL (= 1) */
  const float* shift;      /* [Cout] or NULL (= 0): BN shift, or the repeated ConvTranspose2d bias */
  int32_t relu;            /* 1: ReLU after the affine */
  void* out;               /* NHWC [B, H, W, Cout], storage dtype */
  int32_t B, H, W, Cout;   /* output size; Cout a multiple of 64; H, W even with LD_SEG_SRC_CAT_D2S */
  int32_t dtype;
} ld_seg_conv_args;
int ld_seg_conv(const ld_seg_conv_args* args, void* stream);
/* inc's first convolution (unet_model.py:224): NCHW fp32 image [B, Cin (1 or 3), H, W], OIHW fp32 weight [64, Cin, 3, 3]
 * -> NHWC [B, H, W, 64] storage dtype, the same BN + ReLU epilogue (scale / shift [64]). */
int ld_seg_conv_image(const float* x_nchw, const float* w_oihw, const float* scale, const float* shift, void* out,
                      int B, int Cin, int H, int W, int dtype, void* stream);
/* outc (unet_model.py:209-215, n_classes = 1): NHWC [B, H, W, C] -> logits [B, 1, H, W] fp32 = x . w[C] + bias[0];
 * optionally prob = 1 / (1 + exp(-logit)) (nn.Sigmoid) and mask = (prob > 0.5) as 0 / 1 (test.py:286-288), both
 * [B, 1, H, W] fp32.  Any of the three outputs may be NULL (not all). */
int ld_seg_head(const void* x, const float* w, const float* bias, float* logits, float* prob, float* mask,
                int B, int H, int W, int C, int dtype, void* stream);
/* Weight repacks (fp32, once per model): OIHW [Cout, Cin, k, k] -> [k*k][Cin][Cout]; ConvTranspose2d [Cin, Cout, 2, 2]
 * -> [Cin][(p1, p2, c)] with the bias [Cout] repeated 4x into bias_out [4*Cout] (bias may be NULL: zeros). */
int ld_seg_pack_weight(const float* w_oihw, float* out, int cout, int cin, int ksize, void* stream);
int ld_seg_pack_convt(const float* w, const float* bias, float* w_out, float* bias_out, int cin, int cout, void* stream);

/* ---- training the segmentation U-Net (train_seg.py:78-95): csrc/segtrain.hip -------------------------------------------
 * One optimisation step in fp32, NHWC.  The training-mode forward and the data gradient of every convolution are
 * ld_pc_conv launches (scale = 1, shift = 0 or the ConvTranspose2d bias, no ReLU; the data gradient reads the weight
 * flipped in (ky, kx) and transposed in (Cout, Cin), see ld_seg_permute3).  The entry points below are the rest of the
 * step.  None allocates: reductions take a scratch buffer of LD_SEG_RED_WORK_BYTES, and every reduction adds its partial
 * results in a fixed order (no floating-point atomics), so a step is reproducible bit for bit. */
#define LD_SEG_RED_WORK_BYTES (2048 * 2 * 64 * 8)   /* `work` of the per-channel reductions and of ld_seg_loss */
/* Weight gradient of a 3x3 (pad 1) or 1x1 convolution without bias: dw [Cout][ksize][ksize][Cin] (the OHWI layout
 * ld_pc_conv reads) = sum over pixels of dy [B, H, W, Cout] x a [B, H, W, Cin] shifted by the tap, zero outside the
 * image.  An implicit GEMM on v_mfma_f32_32x32x2_f32 (exact f32) with the pixel axis cut into `splits` parts, each
 * writing its own slab of work [splits][Cout * ksize^2 * Cin], which a second kernel adds in order.  Cin, Cout multiples
 * of 64; 1 <= splits <= ceil(B H W / 32).  ld_seg_wgrad_splits is the split count that fills the chip (0 for a shape
 * ld_seg_wgrad refuses).  ksize 1 with dy = the gradient of the (p1, p2, c) GEMM output is ConvTranspose2d(2, 2)'s. */
int ld_seg_wgrad_splits(int B, int H, int W, int Cin, int Cout, int ksize);
int ld_seg_wgrad(const float* dy, const float* a, float* work, float* dw, int B, int H, int W, int Cin, int Cout,
                 int ksize, int splits, void* stream);
/* BatchNorm2d in training mode + ReLU over y [M, C] (M = B H W values per channel, at least 2; C a multiple of 64):
 * stat [3][C] = batch mean, biased variance, 1 / sqrt(var + eps) (sums in fp64); out = relu((y - mean) invstd gamma +
 * beta); running_mean / running_var (both or neither) updated as nn.BatchNorm2d does, the variance unbiased. */
int ld_seg_bn_train(const float* y, const float* gamma, const float* beta, double* work, float* stat, float* running_mean,
                    float* running_var, float momentum, float eps, float* out, int64_t M, int C, void* stream);
/* Backward of the above: g = da * (act > 0) with act the SAVED activation, dbeta = sum g, dgamma = sum g x^,
 * dy = gamma invstd (g - dbeta / M - x^ dgamma / M).  dy may be da (in place). */
int ld_seg_bn_backward(const float* da, const float* act, const float* y, const float* gamma, const float* stat, double* work,
                       float* dgamma, float* dbeta, float* dy, int64_t M, int C, void* stream);
/* out [C / fold] = sum over the M rows of x [M, C] and over the `fold` groups of C / fold channels (fold 4: the bias
 * gradient of a ConvTranspose2d(2, 2) from the gradient of its (p1, p2, c) GEMM output).  C a multiple of 64. */
int ld_seg_colsum(const float* x, double* work, float* out, int64_t M, int C, int fold, void* stream);
/* MaxPool2d(2): x [B, 2H, 2W, C] -> out [B, H, W, C], and its backward: dx [B, 2H, 2W, C] = dskip (NULL: 0) + dpool at
 * the first maximum of each window in row-major order (ATen's rule).  C a multiple of 4. */
int ld_seg_pool(const float* x, float* out, int B, int H, int W, int C, void* stream);
int ld_seg_pool_backward(const float* x, const float* dpool, const float* dskip, float* dx, int B, int H, int W, int C,
                         void* stream);
/* out [B, H, W, C0 + C1] = cat([skip [B, H, W, C0], depth_to_space(low [B, H/2, W/2, 4*C1])]) (LD_SEG_SRC_CAT_D2S made
 * real), and the split of its gradient into the two parts.  H, W even; C0, C1 multiples of 4. */
int ld_seg_cat_d2s(const float* skip, const float* low, float* out, int B, int H, int W, int C0, int C1, void* stream);
int ld_seg_cat_d2s_backward(const float* dcat, float* dskip, float* dlow, int B, int H, int W, int C0, int C1, void* stream);
/* train_seg.py:89 over M logits: out [3] = {loss, bce, dice loss}, bce = BCEWithLogitsLoss(pos_weight) (mean), dice loss
 * = 1 - (2 sum p t + eps) / (sum p + sum t + eps) with p = sigmoid(logit) over the whole batch, loss = their sum; dz [M]
 * (or NULL) = d loss / d logit.  Sums in fp64. */
int ld_seg_loss(const float* logits, const float* target, double* work, float* out, float* dz, int64_t M, float pos_weight,
                float dice_eps, void* stream);
/* outc backward: dw [C] = sum_p dz[p] x[p, c], db [1] = sum dz, dx [M, C] = dz[p] w[c].  C a multiple of 64. */
int ld_seg_head_backward(const float* dz, const float* x, const float* w, double* work, float* dw, float* db, float* dx,
                         int64_t M, int C, void* stream);
/* torch.optim.Adam's update (no weight decay, no amsgrad) of `count` parameter tensors, 1 .. LD_SEG_ADAM_MAX, in
 * ceil(count / LD_SEG_ADAM_GROUP) launches: a group's table travels by value as the kernel argument (152-byte entries, 16
 * within the 4 KB argument block); nothing is allocated, and the whole table is validated before the first launch.  Each
 * tensor is seen as [d0][d1][d2] (param, m, v contiguous); its gradient element sits at i0 gs0 + i1 gs1 + i2 gs2 of grad;
 * the updated value is also written to mirror0 / mirror1 (or NULL) at off + i0 s0 + i1 s1 + i2 s2 as ld_seg_permute3
 * would: the kernel-layout weight copies stay current without a repack.  step_size = lr / (1 - beta1^t) and bc2_sqrt =
 * sqrt(1 - beta2^t) come from the host in double; 1 - beta is rounded to fp32 once, as torch does. */
#define LD_SEG_ADAM_GROUP 16
#define LD_SEG_ADAM_MAX 1024
typedef struct ld_seg_adam_tensor {
  float* param;
  const float* grad;
  float* m;
  float* v;
  int32_t d0, d1, d2;
  int64_t gs0, gs1, gs2;
  float* mirror0;
  int64_t m0_off, m0_s0, m0_s1, m0_s2;
  float* mirror1;
  int64_t m1_off, m1_s0, m1_s1, m1_s2;
} ld_seg_adam_tensor;
int ld_seg_adam(const ld_seg_adam_tensor* tensors, int count, double beta1, double beta2, double eps, double step_size,
                double bc2_sqrt, void* stream);
/* out[off + i0 s0 + i1 s1 + i2 s2] = in[(i0 d1 + i1) d2 + i2]: the weight layouts of the training step from the
 * parameters' own (OIHW -> OHWI; OIHW -> the data gradient's [Cin][2 - ky][2 - kx][Cout] with a negative stride). */
int ld_seg_permute3(const float* in, float* out, int d0, int d1, int d2, int64_t off, int64_t s0, int64_t s1, int64_t s2,
                    void* stream);

/* ---- PatchCore: the default OOD anomaly-map producer in front of sample() ----------------------------------------------
 * PatchcoreModel (models.py:42-254, eval) with the wide_resnet50_2 trunk up to layer3: features after layer2 / layer3,
 * AvgPool2d(3, 1, 1), bilinear resample of layer3 onto the layer2 grid, concat -> [N, 1536] rows, nearest neighbour in
 * the memory bank, the image score of models.py:222-254 and anomalib's AnomalyMapGenerator (nearest upsample + 33x33
 * Gaussian blur, sigma 4, reflect padding).  Everything is fp32 in storage and arithmetic; activations are NHWC.
 * Convolutions carry BatchNorm (eval) as out = relu?(acc * scale[c] + shift[c] (+ residual)), the affine host-made from
 * the running statistics (the weights are not scaled).  The GEMMs run on v_mfma_f32_32x32x2_f32 (exact f32). */
typedef struct ld_pc_conv_args {
  const float* src;        /* NHWC [B, Hi, Wi, Cin], Cin a multiple of 32 */
  const float* weight;     /* fp32 [Cout][ksize][ksize][Cin] (OIHW permuted to OHWI) */
  const float* scale;      /* [Cout] */
  const float* shift;      /* [Cout] */
  const float* residual;   /* NHWC [B, Ho, Wo, Cout] added after the affine, before the ReLU; or NULL */
  float* out;              /* NHWC [B, Ho, Wo, Cout], Cout a multiple of 64 */
  int32_t B, Hi, Wi, Cin, Ho, Wo, Cout;
  int32_t ksize;           /* 1 (pad 0) or 3 (pad 1); Ho = (Hi + 2 pad - ksize) / stride + 1, likewise Wo */
  int32_t stride;          /* 1 or 2 */
  int32_t relu;
} ld_pc_conv_args;
int ld_pc_conv(const ld_pc_conv_args* args, void* stream);
/* The stem: conv1 7x7 s2 p3 (3 -> 64) from the NCHW fp32 image, bn1 + ReLU -> NHWC [B, Ho, Wo, 64] with
 * Ho = (H - 1) / 2 + 1; w is the OIHW weight [64, 3, 7, 7]. */
int ld_pc_stem(const float* x_nchw, const float* w_oihw, const float* scale, const float* shift, float* out,
               int B, int H, int W, void* stream);
/* MaxPool2d(3, 2, 1): NHWC [B, H, W, C] -> [B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C], C a multiple of 4. */
int ld_pc_maxpool(const float* x, float* out, int B, int H, int W, int C, void* stream);
/* The embedding (models.py:98-102, 129-145, 147-162): AvgPool2d(3, 1, 1) (count_include_pad: / 9) of layer2 [B, h2, w2,
 * C2] and of layer3 [B, h3, w3, C3], bilinear (align_corners=False) resample of the pooled layer3 to h2 x w2, concat ->
 * rows [B*h2*w2, C2 + C3] in (b, y, x) order, and each row's |x|^2 into norms [B*h2*w2].  C2, C3 multiples of 4. */
int ld_pc_embed(const float* l2, const float* l3, float* rows, float* norms, int B, int h2, int w2, int C2, int h3,
                int w3, int C3, void* stream);
/* |x|^2 of each of the n rows of x [n, d] (the memory bank's norms, once per bank). */
int ld_pc_row_norms(const float* x, float* norms, int64_t n, int d, void* stream);
/* Nearest bank row of every query (models.py:179-217, n_neighbors = 1): d2 = (|q|^2 - 2 q.m) + |m|^2, clamped at 0, its
 * min and first argmin over the M rows of bank [M, D] without materialising the N x M matrix.  Query tiles of 128 rows,
 * the bank split over workgroups, merged with a 64-bit atomicMin on (d2 bits << 32 | index).  work: [N] uint64 scratch.
 * dist [N] = sqrt(min d2), idx [N] int32.  D a multiple of 32, M < 2^31. */
int ld_pc_knn(const float* q, const float* qn, int N, const float* bank, const float* bn, int64_t M, int D,
              unsigned long long* work, float* dist, int32_t* idx, void* stream);
/* The k nearest bank rows of each query (k <= 16, topk(largest=False): ascending, the lower index first on equal
 * distances): d2 [N, M] fp32 scratch, dist [N, k] = sqrt(d2), idx [N, k] int32.  k <= M. */
int ld_pc_knn_topk(const float* q, const float* qn, int N, const float* bank, const float* bn, int64_t M, int D, int k,
                   float* d2, float* dist, int32_t* idx, void* stream);
/* ---- the same search with the fp16 matrix cores as a screen (PatchCore.knn_precision = "fp16"), csrc/knn16.hip ----
 * The result is an fp32 search's: the screen only selects the rows that an exact fp32 re-rank looks at, inside a
 * window that its worst-case error bound certifies; what cannot be certified is searched by ld_pc_knn's kernel. */
#define LD_PC_KNN16_CAND 64   /* candidate rows kept per query; more inside the window: that query falls back */
/* Once per bank: bank [M, D] -> bank_hi = fp16(bank), bank_lo = fp16(bank - bank_hi), both fp16 [M, D] (4 M D bytes in
 * all, on top of the fp32 bank, which the re-rank and ld_pc_score* keep using), and info [2] fp32: the largest of
 * bn [M] (the |m|^2 of ld_pc_row_norms), and 1.0 when every element is finite in fp16 (|x| <= 65504), else 0.0 -- such a
 * bank must not be given to ld_pc_knn16.  bank, bank_hi, bank_lo 16-byte aligned, D a multiple of 32, M < 2^31. */
int ld_pc_pack_bank16(const float* bank, const float* bn, int64_t M, int D, void* bank_hi, void* bank_lo, float* info,
                      void* stream);
/* Bytes of scratch for N queries of D elements (their fp16 split, keys, windows, candidate segments). */
int64_t ld_pc_knn16_work_bytes(int N, int D);
/* ld_pc_knn's contract and refusals.  For every query, idx is the argmin (lowest index on ties) and dist the square
 * root of the minimum over ALL M rows of r = max((qn - 2 dot32) + bn, 0), dot32 the fp32 dot product in the re-rank's
 * fixed order; for a query that could not be certified (more than LD_PC_KNN16_CAND rows inside its window, a non-finite
 * window or norm, an element beyond 65504) exactly what ld_pc_knn returns.  No host synchronisation.  work:
 * ld_pc_knn16_work_bytes(N, D) bytes, 16-byte aligned, as q.  stats: NULL or int32 [4] = queries certified, fallen back
 * (they sum to N), bank rows inside all the windows together, the most inside one (the sum can wrap past 2^31). */
int ld_pc_knn16(const float* q, const float* qn, int N, const float* bank, const void* bank_hi, const void* bank_lo,
                const float* bn, const float* info, int64_t M, int D, void* work, float* dist, int32_t* idx,
                int32_t* stats, void* stream);
/* Test instrument, not a production path: the screened distances s [N, M] themselves, for small N x M (the hardware
 * check of the error bound that the window rests on). */
int ld_pc_knn16_screen(const float* q, const float* qn, int N, const void* bank_hi, const void* bank_lo, const float* bn,
                       int64_t M, int D, void* work, float* s_out, void* stream);
/* Image score, part 1 (models.py:241-246): per image the first argmax p* of its P patch scores, and bank row m* = loc[p*]
 * copied to q [B, D] with its norm to qn [B] (the query of the support search).  argmax [B] int32. */
int ld_pc_score_prepare(const float* patch_scores, const int32_t* loc, const float* bank, const float* bn, int B, int P,
                        int D, float* q, float* qn, int32_t* argmax, void* stream);
/* Part 2 (:247-254): distances from row p* of rows [B*P, D] (norms row_norms) to the k support rows support [B, k] of
 * the bank, pred_score[b] = (1 - softmax(d)[0]) * s*.  k = 0: pred_score = max patch score (num_neighbors == 1). */
int ld_pc_score(const float* rows, const float* row_norms, const float* patch_scores, const int32_t* argmax,
                const float* bank, const float* bn, const int32_t* support, int B, int P, int D, int k, float* pred_score,
                void* stream);
/* AnomalyMapGenerator: nearest upsample of the patch scores [B, h, w] to [B, H, W], then the ks-tap Gaussian g (ks odd,
 * reflect padding ks / 2 < min(H, W)) along x into tmp and along y into out, both [B, H, W] fp32. */
int ld_pc_anomaly_map(const float* scores, const float* g, int ks, float* tmp, float* out, int B, int h, int w, int H,
                      int W, void* stream);

/* ---- PatchCore memory banks: anomalib's KCenterGreedy coreset (models.py:165-172), csrc/coreset.hip ---- */
/* The projection F = E @ R^T: E [N, D] row-major (D a multiple of 4, at most 2048), R [k, D] in CSR form (rowptr [k + 1],
 * cols / vals [rowptr[k]]; any R, dense ones included), written feature-major: out [k, ld], ld >= N a multiple of 4,
 * columns N..ld-1 untouched.  E and out 16-byte aligned. */
int ld_pc_project(const float* e, int64_t N, int D, const int32_t* rowptr, const int32_t* cols, const float* vals, int k,
                  float* out, int64_t ld, void* stream);
/* The greedy selection over features ft [k, ld] (the layout of ld_pc_project, 16-byte aligned): min_d = dist(F, F[start]),
 * then n times idx = first argmax(min_d), min_d[idx] = 0, min_d = minimum(min_d, dist(F, F[idx])) with dist the
 * F.pairwise_distance |x - c + 1e-6|_2.  One launch per step on `stream`, no host synchronisation.  min_d: [ld] fp32
 * scratch (16-byte aligned), keys: [n] uint64 scratch (zeroed here), idx: [n] int64, the picks in order.
 * 1 <= n <= N < 2^31, 0 <= start < N, 1 <= k <= 8192. */
int ld_pc_coreset(const float* ft, int64_t ld, int64_t N, int k, int64_t n, int64_t start, float* min_d,
                  unsigned long long* keys, int64_t* idx, void* stream);

/* ---- the hallucination gate around PatchCore (Classifier_PatchCore, models.py:257-430), csrc/classifier.hip ---- */
/* Max of each of the `groups` rows of x [groups, n] fp32 (groups = 1: the whole tensor, models.py:408; groups = B: each
 * sample), accumulated into words[g] with atomicMax on an order-preserving uint32 code of the float.  words must be 0
 * (the code's identity) on entry: ld_clf_resize zeroes a set of words for the next call (zero_words). */
int ld_clf_max(const float* x, int groups, int64_t n, uint32_t* words, void* stream);
enum { LD_CLF_PLAIN = 0, LD_CLF_HALVE = 1, LD_CLF_AFFINE = 2 };
/* Bilinear resize (align_corners=False, no antialiasing, torch's source-index rule) of NCHW fp32 x [B, Cin, Hi, Wi] to
 * out [B, Cout, Ho, Wo]; Cin == Cout, or Cin == 1 read for every output channel (models.py:405-406 without the repeat).
 * mode LD_CLF_HALVE: a sample is halved when the max that ld_clf_max left in max_words[per_sample ? b : 0] is above 1.0
 * (:407-409); LD_CLF_AFFINE: every input value becomes ((v - sub) * mul + add) / div first (:411-422).  normalize: the
 * output is (v - mean[c]) / std[c] (Cout == 3; transforms.Normalize, :424).  zero_words / n_zero: words to clear for the
 * next call's ld_clf_max, or NULL / 0.  pred / threshold / decision / n_decision: also write decision[i] = pred[i] >
 * threshold (int32 1 / 0, :428-430) for i < n_decision; pred NULL: no decision.  One launch, no host synchronisation. */
typedef struct ld_clf_resize_args {
  const float* x;
  float* out;
  int32_t B, Cin, Cout, Hi, Wi, Ho, Wo;
  int32_t mode;
  const uint32_t* max_words;
  int32_t per_sample;
  uint32_t* zero_words;
  int32_t n_zero;
  float sub, mul, add, div;
  int32_t normalize;
  float mean[3], std[3];
  const float* pred;
  float threshold;
  int32_t* decision;
  int32_t n_decision;
} ld_clf_resize_args;
int ld_clf_resize(const ld_clf_resize_args* args, void* stream);
/* decision[i] = pred_score[i] > threshold ? 1 : 0 for i < n, on its own (when no map is resized back). */
int ld_clf_decide(const float* pred_score, float threshold, int32_t* decision, int n, void* stream);

/* ---- the MNIST digit classifier and its training step (train_mnist_cls.py: SimpleCNN), csrc/mnistcls.hip ----------------
 * conv1 (1 -> 32) + ReLU + pool, conv2 (32 -> 64) + ReLU + pool, fc1 (3136 -> 128) + ReLU, fc2 (128 -> 10), softmax
 * cross-entropy (mean), Adam.  fp32, activations NHWC.  conv2 and its two gradients are ld_pc_conv / ld_seg_wgrad launches
 * on a pooled map that carries conv1's 32 channels with a stride of 64 (the upper 32 stay zero); fc1 reads the features in
 * NHWC order (y, x, c), its weight repacked from the reference's (c, y, x).  Every reduction adds in a fixed order (no
 * floating-point atomics).  The optimiser step is ld_seg_adam, whose mirrors keep the repacked weights current. */
/* conv1 + bias + ReLU + MaxPool2d(2): x [B, 28, 28] (one channel), w [32][9], bias [32] -> out [B, 14, 14] pixels of 64
 * floats (only the first 32 are written) and idx [B, 14, 14, 32] (or NULL): the position 0..3 of the first maximum of each
 * 2x2 window in row-major order. */
int ld_mc_conv1(const float* x, const float* w, const float* bias, float* out, unsigned char* idx, int B, void* stream);
/* MaxPool2d(2): x [B, 2H, 2W, C] -> out [B, H, W, C] and idx (or NULL) as above; its backward: dx [B, 2H, 2W, C] = dpool
 * at the stored position where the pooled value (a ReLU output) is positive, 0 elsewhere (ReLU's gradient at 0 is 0). */
int ld_mc_pool(const float* x, float* out, unsigned char* idx, int B, int H, int W, int C, void* stream);
int ld_mc_pool_backward(const float* dpool, const float* pooled, const unsigned char* idx, float* dx, int B, int H, int W,
                        int C, void* stream);
/* out[z][m cm + n] = sum over the K range of split z of a[m am + k ak] * b[n bn + k bk], m < M, n < N, on
 * v_mfma_f32_32x32x2_f32 (exact f32); slab z starts at z M cm.  splits 1 writes the product itself.  Strides in floats,
 * positive; cm >= N; 1 <= splits <= ceil(K / 32), every split owning whole chunks of 32 and at least one. */
int ld_mc_gemm(const float* a, const float* b, float* out, int M, int N, int K, int64_t am, int64_t ak, int64_t bn, int64_t bk,
               int64_t cm, int splits, void* stream);
/* h [B][N] = relu(work[0] + work[1] + ... in order + bias[n]) over the `splits` slabs [B][N] of an ld_mc_gemm. */
int ld_mc_fc1_finish(const float* work, const float* bias, float* h, int B, int N, int splits, void* stream);
/* fc2 and the loss: h [B][128], w2 [10][128], b2 [10] -> logits [B][10], pred [B] (or NULL: the lowest index of the largest
 * logit).  With label [B] (int64; NULL: inference): loss_b [B] = logsumexp(z) - z[label] (the row maximum subtracted),
 * dz [B][10] = (softmax - onehot) / B, dh [B][128] = dz . w2 where h > 0.  A label outside 0..9 indexes nothing: its
 * loss_b is NaN, its dz and dh are 0 and *bad_label is set to 1 (never cleared here). */
int ld_mc_head(const float* h, const float* w2, const float* b2, const int64_t* label, float* logits, int64_t* pred,
               float* loss_b, float* dz, float* dh, int32_t* bad_label, int B, void* stream);
/* gw2 [10][128] = dz^T h, gb2 [10] = sum_b dz, gb1 [128] = sum_b dh (fc1's bias), loss [1] = mean of loss_b. */
int ld_mc_small_grads(const float* dz, const float* h, const float* dh, const float* loss_b, float* gw2, float* gb2, float* gb1,
                      float* loss, int B, void* stream);
/* conv1's weight [32][9] and bias [32] gradient from dp1 (the gradient of ld_mc_conv1's out, same layout), out itself
 * (the ReLU mask) and idx; work holds ld_mc_conv1_wgrad_work_floats(B) floats. */
int64_t ld_mc_conv1_wgrad_work_floats(int B);
int ld_mc_conv1_wgrad(const float* x, const float* p1, const float* dp1, const unsigned char* idx, float* work, float* gw,
                      float* gb, int B, void* stream);

/* ---- training the denoiser, first slice (backward half): csrc/denoiser_grad.hip ----------------------------
 * The gradient of the training loss with respect to the denoiser's output, and the pieces of a trainable ResnetBlock
 * (ddpm.py:170-212) that are not convolutions.  fp32, activations NHWC with a pixel stride ldc >= C: channels C..ldc-1
 * are padding, never read into a statistic or a gradient and written as zeros (what lets ld_pc_conv / ld_seg_wgrad serve
 * a channel count that is a multiple of 32 only).  Every reduction adds in a fixed order with fp64 partial sums (no
 * floating-point atomics); nothing allocates. */
/* Backward of ld_p_losses followed by the batch mean (ddpm.py:1201): d_model_out[b, i] = g * 2 * loss_weight[t_b] *
 * (model_out[b, i] - target[b, i]) / (B * elems_per_sample), target as in ld_p_losses; g = the upstream scalar. */
int ld_p_losses_grad(const float* model_out, const float* x_start, const float* noise, const int* t, const float* sqrt_ab,
                     const float* sqrt_1mab, const float* loss_weight, float g, float* d_model_out, int B,
                     int64_t elems_per_sample, int objective, void* stream);
/* The same with the upstream scalar g * *dev_scale: dev_scale points at one float in device memory, the loss scale of
 * ld_dn_scaler_state (amp = "fp16"); nothing waits for it. */
int ld_p_losses_grad_scaled(const float* model_out, const float* x_start, const float* noise, const int* t, const float* sqrt_ab,
                            const float* sqrt_1mab, const float* loss_weight, float g, const float* dev_scale, float* d_model_out,
                            int B, int64_t elems_per_sample, int objective, void* stream);
/* Bytes of the `work` scratch of the two entry points below (0 for a shape they refuse). */
int64_t ld_dn_gn_work_bytes(int B, int H, int W, int C);
/* GroupNorm (training mode: statistics of this batch) -> FiLM -> SiLU over y [B, H, W, ldc] (a convolution output, bias
 * added): stat [B][groups][2] = (mean, 1 / sqrt(biased var + 1e-5)), out = silu(((y - mean) rstd gamma + beta) (1 + s) +
 * sh) + residual, (s, sh) the halves of film [B][2 C].  film NULL: s = sh = 0; residual ([B, H, W, ldc]) NULL: none; out
 * may be residual.  C a multiple of 4 * groups, ldc a multiple of 4, pointers 16-byte aligned. */
int ld_dn_gn_forward(const float* y, const float* gamma, const float* beta, const float* film, const float* residual,
                     double* work, float* stat, float* out, int B, int H, int W, int C, int ldc, int groups, void* stream);
/* The same with out in bf16 (act_storage = "bf16": an activation only convolutions read), [B, H, W, ldc] at the same pixel
 * stride in elements: the fp32 value above, rounded to nearest even as the bf16 convolutions round an fp32 activation; the
 * padding is zeros, stat is unchanged.  residual stays fp32 and cannot be out.  out_bf16 16-byte aligned. */
int ld_dn_gn_forward_to16(const float* y, const float* gamma, const float* beta, const float* film, const float* residual,
                          double* work, float* stat, void* out_bf16, int B, int H, int W, int C, int ldc, int groups,
                          void* stream);
/* Its backward from dout (the gradient of silu(a)), the saved y and stat; a is recomputed.  dgamma, dbeta [C], dfilm
 * [B][2 C] (NULL exactly when film is), dy [B, H, W, ldc] (may be dout).  One reduction pass over dout and y, a
 * finalisation, one elementwise pass. */
int ld_dn_gn_backward(const float* dout, const float* y, const float* stat, const float* gamma, const float* beta,
                      const float* film, double* work, float* dgamma, float* dbeta, float* dfilm, float* dy, int B, int H,
                      int W, int C, int ldc, int groups, void* stream);
/* The three GroupNorm entry points on a y that is bf16 in memory (conv_out_storage = "bf16": the output of a convolution's
 * _to16 launch), [B, H, W, ldc] at the same pixel stride in elements, 16-byte aligned, its padding never read.  A bf16
 * widens to fp32 exactly, and thread map and the order of every sum are those of the fp32 kernels: the results are bit
 * for bit what the fp32 entry point gives on the widened tensor.  Everything else -- stat, residual, dout, dy (may be
 * dout), the gradients -- stays fp32; _from16_to16 writes out as ld_dn_gn_forward_to16 does (residual cannot be out). */
int ld_dn_gn_forward_from16(const void* y_bf16, const float* gamma, const float* beta, const float* film, const float* residual,
                            double* work, float* stat, float* out, int B, int H, int W, int C, int ldc, int groups,
                            void* stream);
int ld_dn_gn_forward_from16_to16(const void* y_bf16, const float* gamma, const float* beta, const float* film,
                                 const float* residual, double* work, float* stat, void* out_bf16, int B, int H, int W, int C,
                                 int ldc, int groups, void* stream);
int ld_dn_gn_backward_from16(const float* dout, const void* y_bf16, const float* stat, const float* gamma, const float* beta,
                             const float* film, double* work, float* dgamma, float* dbeta, float* dfilm, float* dy, int B, int H,
                             int W, int C, int ldc, int groups, void* stream);
/* out [C] = the sum of x [B, H, W, ldc] over batch and pixels, channels 0..C-1 (the bias gradient of a convolution from
 * the gradient of its output; ld_seg_colsum's sibling with a pixel stride, B x runs workgroups per 256 channels instead
 * of one column of workgroups per 64).  work: ld_dn_gn_work_bytes(B, H, W, C) bytes.  C, ldc multiples of 4. */
int ld_dn_colsum(const float* x, double* work, float* out, int B, int H, int W, int C, int ldc, void* stream);
/* The time projection of a ResnetBlock (ddpm.py:192-195): film [B][N] = silu(temb [B][T]) w[N][T]^T + bias, and its
 * backward: dw = dfilm^T silu(temb), db = sum_b dfilm, dtemb = (dfilm w) * silu'(temb). */
int ld_dn_time_proj(const float* temb, const float* w, const float* bias, float* film, int B, int T, int N, void* stream);
int ld_dn_time_proj_backward(const float* dfilm, const float* temb, const float* w, float* dw, float* db, float* dtemb, int B,
                             int T, int N, void* stream);
/* out [B, H, W, ldc] (channels C..ldc-1 zero) from a tensor [B, C, H, W] with strides (sb, sc, sh, sw) in floats. */
int ld_dn_pack_nhwc(const float* x, float* out, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                    int ldc, void* stream);
/* The same with out in bf16 (rounded to nearest even, the padding zero); ldc even, out_bf16 4-byte aligned. */
int ld_dn_pack_nhwc_to16(const float* x, void* out_bf16, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                         int64_t sw, int ldc, void* stream);
/* out [d0][d1][d2] (contiguous) = in[off + i0 s0 + i1 s1 + i2 s2]: the inverse of ld_seg_permute3 (a padded OHWI weight
 * gradient back to the parameter's OIHW). */
int ld_dn_gather3(const float* in, float* out, int d0, int d1, int d2, int64_t off, int64_t s0, int64_t s1, int64_t s2,
                  void* stream);

/* ---- training the denoiser, second slice: csrc/linattn_grad.hip ------------------------------------------------------------
 * What a trainable LinearAttention (ddpm.py:214-251) needs besides its two 1x1 convolutions: RMSNorm (ddpm.py:126-132) and
 * the attention core, each with its backward.  fp32, the layout above: activations NHWC with a pixel stride, the padding
 * never read into a sum and written as zeros.  qkv is [B, H, W, ld3] with q at channel 0, k at hidden = 32 heads, v at
 * 2 hidden, a head's 32 channels contiguous at 32 head inside each; the attention output and its gradient are [B, H, W,
 * ldo].  Every sum over pixels is added in a fixed order (fp64 across tiles of 64 pixels, parts and samples), the number
 * of parts depends on the shape alone, there are no floating-point atomics and nothing allocates.  Every activation
 * pointer is 16-byte aligned; C, ldc, ld3, ldo are multiples of 4. */
/* Bytes of ld_dn_rms_backward's `work` (0 for a shape it refuses). */
int64_t ld_dn_rms_work_bytes(int B, int H, int W, int C);
/* out [B, H, W, ldc] = x r g[c] sqrt(C) with r = 1 / max(|x_p|_2, 1e-12) over the C real channels of pixel p (an all-zero
 * pixel gives zeros); rinv [B H W] = r, what the backward wants (NULL: not stored). */
int ld_dn_rms_forward(const float* x, const float* g, float* rinv, float* out, int B, int H, int W, int C, int ldc,
                      void* stream);
/* Its backward from dout, the saved x and rinv: with u = x r and e = dout g sqrt(C), dx = r (e - u sum_c u_c e_c) (may be
 * dout) and dg [C] = sqrt(C) sum over batch and pixels of dout_c u_c.  A column-sum pass and its finalisation, then one
 * element-wise pass. */
int ld_dn_rms_backward(const float* dout, const float* x, const float* g, const float* rinv, double* work, float* dg, float* dx,
                       int B, int H, int W, int C, int ldc, void* stream);
/* Parts the pixel axis is cut into by the two reductions below (0 for a refused shape), and the bytes of their `work`. */
int ld_dn_la_splits(int B, int heads, int H, int W);
int64_t ld_dn_la_work_bytes(int B, int heads, int H, int W);
/* The context of every (b, head): kstat [B, heads, 32, 2] = (m[d] = max_n k[d, n], Z[d] = sum_n exp(k[d, n] - m[d])) and
 * ctx [B, heads, 32, 32], ctx[d][e] = sum_n exp(k[d, n] - m[d]) v[e, n] / Z[d].  Every part reduces under its own maximum;
 * a second launch merges the parts in index order, rescaled to the common maximum. */
int ld_dn_la_context(const float* qkv, double* work, float* ctx, float* kstat, int B, int H, int W, int heads, int ld3,
                     void* stream);
/* out[n][32 head + e] = 32^-0.5 sum_d ctx[d][e] softmax_d(q[:, n])[d]; channels 32 heads .. ldo-1 zero. */
int ld_dn_la_out(const float* qkv, const float* ctx, float* out, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
/* The backward's one reduction over pixels, from dout = the gradient of ld_dn_la_out's out: dctx [B, heads, 32, 32],
 * dctx[d][e] = 32^-0.5 sum_n softmax_d(q[:, n])[d] dout[e, n], and rk [B, heads, 32], rk[d] = sum_e dctx[d][e] ctx[d][e]
 * (= sum_n ks[d, n] dks[d, n]: what the backward of the softmax over pixels needs). */
int ld_dn_la_backward_reduce(const float* qkv, const float* dout, const float* ctx, double* work, float* dctx, float* rk, int B,
                             int H, int W, int heads, int ld3, int ldo, void* stream);
/* The backward's element-wise pass: dqkv [B, H, W, ld3] (channels 96 heads .. ld3-1 zero) with, per pixel and head, p =
 * softmax_d(q), ks = exp(k - m) / Z, dq[d] = 32^-0.5 p[d] (s[d] - sum_d' p[d'] s[d']) for s[d] = sum_e ctx[d][e] dout[e],
 * dk[d] = ks[d] (sum_e dctx[d][e] v[e] - rk[d]), dv[e] = sum_d dctx[d][e] ks[d]. */
int ld_dn_la_backward_apply(const float* qkv, const float* dout, const float* ctx, const float* kstat, const float* dctx,
                            const float* rk, float* dqkv, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
/* The same four passes on the bf16 matrix cores (csrc/linattn16.hip; LinearAttention.attn_precision = "bf16"): the same
 * arguments, fp32 tensors, layouts, `work`, parts and refusals.  Both operands of every 32 x 32 product are rounded to bf16
 * (round-to-nearest-even, NaN kept, as ld_dn_conv16 rounds) and multiplied by v_mfma_f32_32x32x16_bf16: exact products, an
 * fp32 accumulator.  Nothing else is rounded; every sum keeps one order, no atomics, nothing allocates.
 * context16: P = exp(k - m_part) is computed in fp32 and then rounded, v is rounded; m and Z are ld_dn_la_context's (Z sums
 * the unrounded P: fp32 inside a run, fp64 across runs); the products leave the fp32 accumulator into fp64 every 16 tiles
 * of 64 pixels, where a wave's accumulator has summed 256 pixels; the fp64 parts and the merge launch are unchanged. */
int ld_dn_la_context16(const float* qkv, double* work, float* ctx, float* kstat, int B, int H, int W, int heads, int ld3,
                       void* stream);
/* out16: p = softmax_d(q) in fp32, then rounded; ctx rounded; the product times 32^-0.5 in fp32. */
int ld_dn_la_out16(const float* qkv, const float* ctx, float* out, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
/* backward_reduce16: p and dout rounded; the merge (32^-0.5, rk from the fp32 dctx and ctx in fp64) is unchanged. */
int ld_dn_la_backward_reduce16(const float* qkv, const float* dout, const float* ctx, double* work, float* dctx, float* rk, int B,
                               int H, int W, int heads, int ld3, int ldo, void* stream);
/* backward_apply16: s = ctx dout, tk = dctx v and dv = dctx^T ks with all six operands rounded; ks, p, the dot product, rk
 * and the three output formulas in fp32 with the unrounded p and ks, as ld_dn_la_backward_apply writes them. */
int ld_dn_la_backward_apply16(const float* qkv, const float* dout, const float* ctx, const float* kstat, const float* dctx,
                              const float* rk, float* dqkv, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
/* The same four passes on the fp16 matrix cores (LinearAttention.amp_attn = "fp16"; the <f16> instantiations of the same
 * kernel templates): the arguments, `work`, parts, refusals and the order of every sum are the ...16 entry points', the
 * operands are rounded to fp16 instead (v_cvt_pk_f16_f32: round-to-nearest-even, no saturation -- beyond 65504 is inf;
 * subnormal operands are kept, nothing is flushed) and multiplied by v_mfma_f32_32x32x16_f16.  One operand pair differs, in
 * backward_apply's dv: ks = exp(k - m) / Z is about 1 / (H W) and would be an fp16 subnormal from 128 x 128 pixels on, so
 *   dv[e] = sum_d fp16(dctx[d][e] (1 / Z[d])) fp16(exp(k[d] - m[d])),
 * the division moved to the dctx side and the second operand in (0, 1]; dk keeps the unrounded fp32 ks.  What can leave
 * fp16's range (a large dout or dctx, q / k / v beyond 65504) becomes inf or underflows: these run under a loss scaler. */
int ld_dn_la_context_f16(const float* qkv, double* work, float* ctx, float* kstat, int B, int H, int W, int heads, int ld3,
                         void* stream);
int ld_dn_la_out_f16(const float* qkv, const float* ctx, float* out, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
int ld_dn_la_backward_reduce_f16(const float* qkv, const float* dout, const float* ctx, double* work, float* dctx, float* rk, int B,
                                 int H, int W, int heads, int ld3, int ldo, void* stream);
int ld_dn_la_backward_apply_f16(const float* qkv, const float* dout, const float* ctx, const float* kstat, const float* dctx,
                                const float* rk, float* dqkv, int B, int H, int W, int heads, int ld3, int ldo, void* stream);

/* ---- training the denoiser, third slice: csrc/attention_grad.hip ------------------------------------------------------------
 * The core of a trainable full Attention (ddpm.py:253-282, attend.py's non-flash path): softmax(q k^T 32^-0.5) v per
 * (sample, head), fp32 with exact fp32 products, on the layout above (qkv [B, H, W, ld3], out / dout [B, H, W, ldo]); q is
 * not pre-scaled.  Nothing of size n x n (n = H W) is written to memory: the forward is an online softmax over tiles of 64
 * keys, the backward recomputes the probabilities from qkv and lse.  Every sum is added in a fixed order, there are no
 * atomics and nothing allocates; padded channels are never read, and written as zeros.  qkv, out, dout and dqkv are 16-byte
 * aligned; ld3 >= 96 heads and ldo >= 32 heads are multiples of 4. */
/* out[n][32 head + e] = sum_j softmax_j(q_n . k_j 32^-0.5) v_j[e], channels 32 heads .. ldo-1 zero; lse [B, heads, n] = the
 * row's max + log of its normaliser, what the backward wants (NULL: not stored). */
int ld_dn_fa_forward(const float* qkv, float* out, float* lse, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
/* Bytes of ld_dn_fa_backward's `work` (delta = rowsum(dout out), [B, heads, n] floats); 0 for a shape it refuses. */
int64_t ld_dn_fa_work_bytes(int B, int heads, int H, int W);
/* dqkv [B, H, W, ld3] (channels 96 heads .. ld3-1 zero) from dout = the gradient of ld_dn_fa_forward's out, with p_nj =
 * exp(q_n . k_j 32^-0.5 - lse_n) and ds_nj = p_nj (dout_n . v_j - delta_n): dq_n = 32^-0.5 sum_j ds_nj k_j, dk_j = 32^-0.5
 * sum_n ds_nj q_n, dv_j = sum_n p_nj dout_n.  A row pass (one workgroup per 64 queries: delta and dq) and a column pass
 * (one per 64 keys: dk and dv). */
int ld_dn_fa_backward(const float* qkv, const float* out, const float* dout, const float* lse, void* work, float* dqkv, int B,
                      int H, int W, int heads, int ld3, int ldo, void* stream);
/* The same passes on the bf16 matrix cores (csrc/attention16.hip; Attention.full_attn_precision = "bf16"): the same
 * arguments, fp32 tensors, layouts, `work` (ld_dn_fa_work_bytes) and refusals.  Both operands of every product are rounded to
 * bf16 (round-to-nearest-even, NaN kept, as ld_dn_conv16 rounds) and multiplied by v_mfma_f32_32x32x16_bf16: exact products,
 * an fp32 accumulator.  forward16: S = q^ k^T, the logits S 32^-0.5, the online softmax (the running maximum, alpha, the
 * normaliser of the UNROUNDED p) and out = O / l in fp32 with ld_dn_fa_forward's formulas; O = p^ v^, p rounded after it is
 * computed.  Every sum keeps one order, no atomics, nothing allocates, nothing of size n x n is written. */
int ld_dn_fa_forward16(const float* qkv, float* out, float* lse, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
/* backward16: p = exp(q^ . k^ 32^-0.5 - lse) and delta = rowsum(dout out) (unrounded) in fp32; dP = dout^ v^T; ds = p (dP -
 * delta) in fp32, then rounded; dq = 32^-0.5 (ds^ k^), dk = 32^-0.5 (ds^T q^), dv = p^T dout^, the scale applied to the fp32
 * sum.  The same two passes as ld_dn_fa_backward. */
int ld_dn_fa_backward16(const float* qkv, const float* out, const float* dout, const float* lse, void* work, float* dqkv, int B,
                        int H, int W, int heads, int ld3, int ldo, void* stream);
/* The same passes on the fp16 matrix cores (Attention.amp_attn = "fp16"; the <f16> instantiations of the same kernel
 * templates): the contract of forward16 / backward16 with fp16 rounding of the same operands (q, k, v, dO, p, ds;
 * v_cvt_pk_f16_f32: round-to-nearest-even, beyond 65504 is inf, subnormals kept) and v_mfma_f32_32x32x16_f16.  A small p or
 * ds underflows and a large dO overflows: these run under a loss scaler. */
int ld_dn_fa_forward_f16(const float* qkv, float* out, float* lse, int B, int H, int W, int heads, int ld3, int ldo, void* stream);
int ld_dn_fa_backward_f16(const float* qkv, const float* out, const float* dout, const float* lse, void* work, float* dqkv, int B,
                          int H, int W, int heads, int ld3, int ldo, void* stream);

/* ---- training the denoiser, fourth slice: csrc/resample_grad.hip -------------------------------------------------------------
 * What the layers between the blocks need besides ld_pc_conv / ld_seg_wgrad / ld_dn_colsum: Downsample's rearrangement
 * (ddpm.py:120-124) and Upsample's nearest x 2 (ddpm.py:114-118), each with its backward, the im2col of the 7 x 7 stem and
 * the head (final_conv).  fp32, the layout above: activations NHWC with a pixel stride ldc >= C, the padding never read and
 * written as zeros.  The layout kernels move 16 bytes per thread; nothing allocates, there are no atomics, every sum has one
 * order.  Activation pointers are 16-byte aligned; C and ldc are multiples of 4 (the head: of 32), ldc <= 65,536, H and W
 * <= 2^20 and B H W <= 2^36.  A refused call returns -1 before anything is launched. */
/* out [B, H, W, 4 C] (no padding), channel (p1 2 + p2) C + c = x [B, 2 H, 2 W, ldc] at (2 h + p1, 2 w + p2, c): the
 * reference's 'b c (h p1) (w p2) -> b (c p1 p2) h w' with the channel order (p1 p2 c), which the weight packing absorbs. */
int ld_dn_space_to_depth(const float* x, float* out, int B, int H, int W, int C, int ldc, void* stream);
/* Its inverse: dx [B, 2 H, 2 W, ldc] (channels C..ldc-1 zero) from g [B, H, W, 4 C]. */
int ld_dn_depth_to_space(const float* g, float* dx, int B, int H, int W, int C, int ldc, void* stream);
/* out [B, 2 H, 2 W, ldc] = x [B, H, W, ldc] at (h / 2, w / 2): F.interpolate(scale_factor=2, mode="nearest"). */
int ld_dn_upsample2x(const float* x, float* out, int B, int H, int W, int C, int ldc, void* stream);
/* Its backward: dx [B, H, W, ldc] = ((g[2h][2w] + g[2h][2w+1]) + g[2h+1][2w]) + g[2h+1][2w+1] from g [B, 2 H, 2 W, ldc],
 * in fp32 and in that order. */
int ld_dn_upsample2x_backward(const float* g, float* dx, int B, int H, int W, int C, int ldc, void* stream);
/* out [B, H, W, ldk], column (ci 7 + ky) 7 + kx = x[b][ci][y + ky - 3][x + kx - 3], zero outside the image and in the
 * columns from 49 Cin on: the 7 x 7 (padding 3) stem as a 1 x 1 convolution whose weight is the OIHW parameter as it lies
 * in memory.  x is [B, Cin, H, W] with strides (sb, sc, sh, sw) in floats, Cin 1..4; ldk >= 49 Cin a multiple of 4. */
int ld_dn_im2col(const float* x, float* out, int B, int Cin, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                 int ldk, void* stream);
/* The head, Conv2d(C, O, 1) with O 1..8 and C <= 2048: out NCHW [B, O, H, W] = sum_c x [B, H, W, ldc] w [O][C] + bias [O] (fp32 sums:
 * a lane's four channels per 32-channel chunk in chunk order, then the eight lanes of a pixel pairwise). */
int ld_dn_head_forward(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C, int ldc,
                       int O, void* stream);
/* Parts the pixels are cut into by ld_dn_head_backward (0 for a refused shape; it depends on B H W alone), and the bytes
 * of its `work`. */
int ld_dn_head_splits(int B, int H, int W);
int64_t ld_dn_head_work_bytes(int B, int H, int W, int C, int O);
/* Its backward from dout NCHW [B, O, H, W]: dx [B, H, W, ldc] = sum_o dout w (o order; channels C..ldc-1 zero), dw [O][C] =
 * sum over pixels of dout x and db [O] = sum of dout: fp64 sums per part, the parts added in index order by a second
 * launch. */
int ld_dn_head_backward(const float* dout, const float* x, const float* w, double* work, float* dw, float* db, float* dx,
                        int B, int H, int W, int C, int ldc, int O, void* stream);

/* ---- training the denoiser, fifth slice: csrc/condenc_grad.hip ----------------------------------------------------------------
 * What a trainable BasicBlock of the ResUnet condition encoder (unet_model.py:8-51) needs besides ld_pc_conv / ld_seg_wgrad /
 * ld_dn_colsum / ld_seg_pool: GroupNorm in training mode at an even number of channels per group (16 groups of 2 at 32
 * channels: a thread's four channels are two pairs, each in one group) followed by ReLU or nothing, of one tensor or of the
 * sum of two normalised tensors, with its backward; and the im2col of a 3 x 3 convolution on an image.  fp32, the layout
 * above: activations NHWC with a pixel stride ldc >= C, the padding never read into a statistic or a gradient and written as
 * zeros (every output is a whole padded tensor).  Sums are fp64 per run of pixels, merged in index order; no atomics, nothing
 * allocates.  Activation, gamma and beta pointers are 16-byte aligned, work 8-byte; C is a multiple of 4 and of 2 groups, C <=
 * 2048, ldc <= 4096 a multiple of 4, B <= 32,767, H and W <= 2^20, B H W <= 2^36.  A refused call returns -1 before anything
 * is launched. */
/* Bytes of the `work` scratch of the two entry points below, either form (0 for a shape they refuse). */
int64_t ld_dn_gnr_work_bytes(int B, int H, int W, int C, int groups);
/* out [B, H, W, ldc] = act(GN(y; gamma, beta) + GN(y2; gamma2, beta2)), act = ReLU when relu != 0 and nothing otherwise, GN
 * with the statistics of this batch: stat (stat2) [B][groups][2] = (mean, 1 / sqrt(biased var + 1e-5)) of y (y2).  y2,
 * gamma2, beta2 and stat2 are all NULL (the one-operand form, convblock.1) or all given (the block's tail). */
int ld_dn_gnr_forward(const float* y, const float* gamma, const float* beta, const float* y2, const float* gamma2,
                      const float* beta2, double* work, float* stat, float* stat2, float* out, int B, int H, int W, int C, int ldc,
                      int groups, int relu, void* stream);
/* Its backward from dout, the saved result act (relu != 0: g = dout where act > 0, else 0 -- ld_seg_bn_backward's rule; relu
 * == 0: g = dout and act may be NULL), the saved y and stat (y2 and stat2): dbeta [C] = sum g, dgamma [C] = sum g y^, dy = rstd
 * (gamma g - mean_group(gamma g) - y^ mean_group(gamma g y^)), and the same for the second operand from the same g (dbeta2 =
 * dbeta).  One reduction pass, a finalisation, one element-wise pass.  dy may be dout; dy2 is a buffer of its own. */
int ld_dn_gnr_backward(const float* dout, const float* act, const float* y, const float* stat, const float* gamma,
                       const float* y2, const float* stat2, const float* gamma2, double* work, float* dgamma, float* dbeta,
                       float* dy, float* dgamma2, float* dbeta2, float* dy2, int B, int H, int W, int C, int ldc, int groups,
                       int relu, void* stream);
/* out [B, H, W, ldk], column (ci 3 + ky) 3 + kx = x[b][ci][y + ky - 1][x + kx - 1], zero outside the image and in the columns
 * from 9 Cin on: a 3 x 3 (padding 1) convolution on an image as a 1 x 1 convolution whose weight is the OIHW parameter as it
 * lies in memory.  x is [B, Cin, H, W] with strides (sb, sc, sh, sw) in floats, Cin 1..4; ldk >= 9 Cin a multiple of 4. */
int ld_dn_im2col3(const float* x, float* out, int B, int Cin, int H, int W, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int ldk,
                  void* stream);

/* ---- training the denoiser, sixth slice: csrc/unet_grad.hip --------------------------------------------------------------------
 * What a trainable Unet (ddpm.py:286-451) needs besides its blocks: the time MLP (sinusoidal embedding -> Linear(dim, T) ->
 * GELU -> Linear(T, T), ddpm.py:136-149 and :339-344) in training form with its backward, and the glue of Unet.forward in the
 * padded NHWC layout.  fp32 data; the time MLP's sums are fp64 in a fixed order (a wave's lanes over the input features, then
 * the shuffle tree; the batch in index order), no atomics, nothing allocates.  A refused call returns -1 before anything is
 * launched. */
/* emb [B, dim] = (sin(times[b] freqs[k]), cos(..)) with times [B] as fp32 and the dim / 2 frequencies made on the host (the
 * reference multiplies a long t by an fp32 table: float(t) * freq); h1 [B, T] = emb w1^T + b1, the pre-GELU value the backward
 * reads; temb [B, T] = gelu(h1) w3^T + b3, the exact (erf) GELU.  w1 [T, dim], w3 [T, T] as nn.Linear keeps them.  dim even and
 * >= 4, T a multiple of 4, dim + T <= 12288; any B >= 1 (a workgroup per sample). */
int ld_dn_time_mlp_forward(const float* times, const float* freqs, const float* w1, const float* b1, const float* w3,
                           const float* b3, float* emb, float* h1, float* temb, int B, int dim, int T, void* stream);
/* Bytes of the `work` scratch of the backward (0 for a shape it refuses): gelu(h1) and dh1, [B, T] floats each. */
int64_t ld_dn_time_mlp_work_bytes(int B, int dim, int T);
/* Its backward from dtemb [B, T] and the saved emb and h1: dw3 [T, T] = dtemb^T gelu(h1), db3 [T] = sum_b dtemb, dh1 = (dtemb
 * w3) gelu'(h1), dw1 [T, dim] = dh1^T emb, db1 [T] = sum_b dh1; `times` has no gradient.  Two launches: an element of dh1 per
 * thread, then an element of a parameter gradient per thread that walks the batch in index order (any B >= 1). */
int ld_dn_time_mlp_backward(const float* dtemb, const float* emb, const float* h1, const float* w3, float* work, float* dw1,
                            float* db1, float* dw3, float* db3, int B, int dim, int T, void* stream);
/* out [B, H, W, ldo]: channels 0..ca-1 = a [B, H, W, lda] (+ a2 of the same stride when given), channels ca..ca+cb-1 = b [B, H,
 * W, ldb] when given (b == NULL goes with cb == 0), the columns from ca + cb to ldo zero.  With b == NULL it is attn(x) + x,
 * with a2 == NULL torch.cat((a, b), dim = channels); one of the two must be given.  ca and cb are multiples of 32, every
 * stride a multiple of 4 floats, every pointer 16-byte aligned: 16-byte loads and stores, and the sources' padding is never
 * read.  Its gradients are views of dout, so there is no backward kernel. */
int ld_dn_join(const float* a, const float* a2, const float* b, float* out, int B, int H, int W, int ca, int lda, int cb, int ldb,
               int ldo, void* stream);

/* ---- training the denoiser, seventh slice: csrc/denoiser_opt.hip ----------------------------------------------------------------
 * The optimiser step of the reference's Trainer.train (ddpm.py:1558-1571) over every parameter tensor of the Unet at once:
 * clip_grad_norm_, Adam, zero_grad and the EMA update in two launches.  The tensors are described by a table in DEVICE memory
 * (a few hundred entries do not fit in kernel arguments), built once per trainer: fill param, count and flags of a HOST array,
 * let ld_dn_opt_layout assign the segments and workgroups, copy the array to the device.  Every tensor owns a 16-byte aligned
 * segment [offset, offset + count) of four flat buffers of flat_floats floats -- grad, exp_avg, exp_avg_sq, ema -- and the
 * workgroups first_wg .. of LD_DN_OPT_CHUNK elements each, so no workgroup straddles two tensors; counts need not be multiples
 * of 4.  An entry without LD_DN_OPT_ADAM has no gradient and no moments (the reference's conv_fusion.mlp.1.*: it is not in the
 * norm and Adam leaves it alone) but is in the EMA.  fp32 storage, fp64 sums in an order that depends on the sizes alone, no
 * atomics, nothing allocates; a refused call returns -1 before anything is launched.  The kernels keep every access to the
 * flat buffers inside flat_floats whatever the table holds; the parameter pointers are the table's. */
#define LD_DN_OPT_CHUNK 4096
#define LD_DN_OPT_MAX_TENSORS 65536
#define LD_DN_OPT_ADAM 1
typedef struct ld_dn_opt_tensor {
  float* param;     /* the parameter's own memory: 4-byte aligned; a 16-byte aligned one takes the 16-byte loads and stores */
  int64_t count;    /* elements, >= 1 */
  int64_t offset;   /* (out) first float of its segment in the flat buffers, a multiple of 4 */
  int32_t first_wg; /* (out) its first workgroup */
  int32_t flags;    /* LD_DN_OPT_ADAM or 0 */
} ld_dn_opt_tensor;
/* Host only: checks param / count / flags of the n_tensors entries and fills offset and first_wg in index order; *flat_floats
 * is the length of each flat buffer, *workgroups the grid of the two entry points below.  Nothing is written when it refuses. */
int ld_dn_opt_layout(ld_dn_opt_tensor* tensors, int n_tensors, int64_t* flat_floats, int64_t* workgroups);
/* *sumsq (device) = the sum of the squares of every gradient segment of an LD_DN_OPT_ADAM entry, in fp64: one partial per
 * workgroup into work (ld_dn_opt_sqnorm_work_bytes(n_wg) bytes), added by a second launch of one workgroup in a fixed order
 * (thread t takes partials t, t + 256, .. in index order; then the wave's shuffle tree and the four waves in order).
 * grad 16-byte aligned, table / work / sumsq 8-byte aligned. */
int64_t ld_dn_opt_sqnorm_work_bytes(int n_wg);
int ld_dn_opt_sqnorm(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, const float* grad, int64_t flat_floats, double* work,
                     double* sumsq, void* stream);
/* Data-parallel training: ld_dn_opt_reduce in the place of ld_dn_opt_sqnorm.  gathered (device) holds `world` copies of the
 * flat gradient, rank r's at gathered + r * rank_stride (what an all-gather of the ranks' buffers leaves).  Per element i of
 * every LD_DN_OPT_ADAM entry: g = gathered[i], then g += gathered[r * rank_stride + i] for r = 1 .. world - 1 -- plain fp32
 * additions in that order, whatever the world size -- and grad[i] = g; the squares of g go into the per-workgroup fp64
 * partials in ld_dn_opt_sqnorm's order, and the same second launch adds them: *sumsq and work hold the bits that
 * ld_dn_opt_sqnorm gives on the reduced buffer.  Entries without LD_DN_OPT_ADAM and the padding between segments are neither
 * read in gathered nor written in grad.  grad is a buffer of its own or one rank's copy (gathered + r * rank_stride): a thread
 * stores only elements it has loaded from every copy.  Refused with -1 before anything is launched: world outside 1 ..
 * LD_DN_OPT_MAX_WORLD, rank_stride below flat_floats or no multiple of 4, gathered or grad off the 16-byte grid (table, work,
 * sumsq: 8 bytes), a grad that overlaps gathered in any other way. */
#define LD_DN_OPT_MAX_WORLD 64
int ld_dn_opt_reduce(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, const float* gathered, int world, int64_t rank_stride,
                     float* grad, int64_t flat_floats, double* work, double* sumsq, void* stream);
/* The loss tail of the same exchange: *out (device) = gathered[at], then += gathered[r * rank_stride + at] for r = 1 ..
 * world - 1, by one thread; 0 <= at < rank_stride.  Nothing else of gathered is read. */
int ld_dn_opt_reduce_tail(const float* gathered, int world, int64_t rank_stride, int64_t at, float* out, void* stream);
/* One launch over the table.  coef = min(1, max_norm / (sqrt(*sumsq) + 1e-6)) (clip_grad_norm_; *sumsq is read on the device,
 * and a NaN norm gives a NaN coef as torch's clamp does); per element of an LD_DN_OPT_ADAM entry ld_seg_adam's update from
 * g coef (step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) from the host in double, 1 - beta rounded to fp32
 * once) and grad = 0; then per element of every entry, with p the updated parameter: ema_mode 0 leaves ema alone, 1 sets
 * ema = p, 2 sets ema = lerp(ema, p, ema_w) as ATen evaluates it (ema + ema_w (p - ema) below ema_w = 0.5, p - (p - ema)
 * (1 - ema_w) from there on).  max_norm >= 0 (infinity: no clipping); 0 <= ema_w <= 1. */
int ld_dn_opt_step(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, float* grad, float* exp_avg, float* exp_avg_sq,
                   float* ema, int64_t flat_floats, const double* sumsq, double max_norm, double beta1, double beta2, double eps,
                   double step_size, double bc2_sqrt, int ema_mode, float ema_w, void* stream);

/* Loss scaling (amp = "fp16"): torch.amp.GradScaler's state and decisions in device memory.  The gradients are produced
 * multiplied by `scale` (ld_p_losses_grad_scaled reads it on the device); ld_dn_opt_sqnorm / ld_dn_opt_reduce give the squared
 * norm of those scaled gradients, which is non-finite exactly when one of them is; ld_dn_opt_scaler_update decides and
 * ld_dn_opt_step_scaled acts, so the host never waits for the decision. */
typedef struct ld_dn_scaler_state {
  float scale;             /* the loss scale the NEXT gradients are produced with */
  int32_t growth_tracker;  /* finite steps in a row since the scale last changed (GradScaler._growth_tracker) */
  int32_t adam_steps;      /* optimiser steps that were not skipped: Adam's own step count */
  int32_t skipped_steps;
  int32_t found_inf;       /* the last step's flag: 1 = it was skipped */
  float inv_scale;         /* (float)(1 / (double)scale) of the scale the last gradients were produced with */
  float step_size;         /* lr / (1 - beta1^adam_steps), rounded to fp32 as ld_dn_opt_step rounds its argument */
  float bc2_sqrt;          /* sqrt(1 - beta2^adam_steps), the same way */
} ld_dn_scaler_state;
/* One thread fills *state (device): scale = init_scale (positive, finite), the two counts as given, skipped_steps = found_inf =
 * 0, inv_scale = 1 / scale. */
int ld_dn_scaler_init(ld_dn_scaler_state* state, float init_scale, int adam_steps, int growth_tracker, void* stream);
/* One thread, between the norm and the step: found_inf = !isfinite(*sumsq); inv_scale from the current scale; a finite norm
 * counts an Adam step and computes step_size and bc2_sqrt for it in fp64 (pow), a non-finite one counts a skipped step; then
 * torch's _amp_update_scale_: found_inf -> scale *= backoff_factor, tracker = 0; else tracker += 1 and at growth_interval
 * scale *= growth_factor (only if the product is finite) and tracker = 0.  growth_factor > 1, 0 < backoff_factor < 1,
 * growth_interval >= 1. */
int ld_dn_opt_scaler_update(ld_dn_scaler_state* state, const double* sumsq, double lr, double beta1, double beta2,
                            double growth_factor, double backoff_factor, int growth_interval, void* stream);
/* ld_dn_opt_step with found_inf, inv_scale, step_size and bc2_sqrt read from *state: coef from sqrt(*sumsq) * inv_scale, the
 * gradient (g * inv_scale) * coef (torch unscales in place, then clips; with a power-of-two scale both products are exact).
 * On found_inf the parameters and both moments keep their bits; either way the gradient is zeroed and the EMA acts. */
int ld_dn_opt_step_scaled(const ld_dn_opt_tensor* table, int n_tensors, int n_wg, float* grad, float* exp_avg, float* exp_avg_sq,
                          float* ema, int64_t flat_floats, const double* sumsq, const ld_dn_scaler_state* state, double max_norm,
                          double beta1, double beta2, double eps, int ema_mode, float ema_w, void* stream);

/* ---- training the denoiser, the convolutions in bf16 (conv_precision = "bf16"): csrc/conv16.hip ---------------------------------
 * ld_pc_conv and ld_seg_wgrad with both operands of every product rounded to bf16 (round-to-nearest-even, NaN kept) and
 * multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Memory keeps its formats: activations, gradients and the
 * weight gradient are fp32; only the kernel-layout copy of a weight is bf16.  No floating-point atomics, nothing allocates,
 * nothing synchronises; a refused call returns -1 before anything is launched. */
/* ld_pc_conv's contract (args->weight is ignored) at stride 1 with weight_bf16 [Cout][ksize][ksize][Cin] in bf16: out = acc *
 * scale + shift (+ residual), then the optional ReLU, fp32 NHWC.  Cin a multiple of 32, Cout of 64, ksize 1 or 3; src and
 * weight_bf16 16-byte aligned.  The data gradient is the same call on the flipped, transposed weight (ld_dn_pack_conv16). */
int ld_dn_conv16(const ld_pc_conv_args* args, const void* weight_bf16, void* stream);
/* ld_seg_wgrad's contract: dw [Cout][ksize][ksize][Cin] fp32 from fp32 dy and a, one slab of work [splits][Cout * ksize^2 *
 * Cin] per split of the pixel axis (a split without pixels writes zeros), added in index order by a second kernel.  Cin, Cout
 * multiples of 64; 1 <= splits <= ceil(B H W / 32) (ld_seg_wgrad_splits gives the count); dy and a 16-byte aligned. */
int ld_dn_wgrad16(const float* dy, const float* a, float* work, float* dw, int B, int H, int W, int Cin, int Cout, int ksize,
                  int splits, void* stream);
/* ld_dn_conv16 and ld_dn_wgrad16 on an activation that is bf16 in memory (act_storage = "bf16"): args->src, or a, points at a
 * bf16 NHWC tensor of the same shape and the same pixel stride in elements, 16-byte aligned; dy, the residual and every
 * output stay fp32.  The loader copies where the fp32 one rounds and everything behind it is the same code, so the result
 * is bit for bit that of the fp32 tensor which rounds to this one; taps outside the image and rows beyond the last pixel are
 * zeros.  Same shapes, same refusals, same work buffer and split count. */
int ld_dn_conv16_from16(const ld_pc_conv_args* args, const void* weight_bf16, void* stream);
int ld_dn_wgrad16_from16(const float* dy, const void* a_bf16, float* work, float* dw, int B, int H, int W, int Cin, int Cout,
                         int ksize, int splits, void* stream);
/* ld_dn_conv16 and ld_dn_conv16_from16 with the OUTPUT in bf16 (conv_out_storage = "bf16"): args->out points at a bf16 NHWC
 * tensor [B, Ho, Wo, Cout], 4-byte aligned.  The epilogue's fp32 value (scale, shift, the optional fp32 residual, relu) is
 * computed by the same code and rounded to nearest even on its way out, so the result is the fp32 entry point's, rounded.
 * Same shapes and refusals; the fp32 residual cannot be out. */
int ld_dn_conv16_to16(const ld_pc_conv_args* args, const void* weight_bf16, void* stream);
int ld_dn_conv16_from16_to16(const ld_pc_conv_args* args, const void* weight_bf16, void* stream);
/* An OIHW fp32 parameter [co][ci][k][k] to the two bf16 kernel layouts in one launch: fwd [cop][k * k][cip] and dgr
 * [cip][k * k, flipped][cop] (dgr[c][k * k - 1 - t][o] = w[o][c][t]), zero in the padded channels.  k 1 or 3; cop >= co and
 * cip >= ci, both even. */
int ld_dn_pack_conv16(const float* w_oihw, void* fwd_bf16, void* dgr_bf16, int co, int cop, int ci, int cip, int k, void* stream);
/* The fp16 forms (amp = "fp16"): ld_dn_conv16, ld_dn_wgrad16 and ld_dn_pack_conv16 with both operands rounded to fp16
 * (round-to-nearest-even; a value beyond 65504 becomes inf, it is not saturated: the loss scaler finds overflows by it), fp16
 * packed weights and v_mfma_f32_32x32x16_f16; the same tiles, order of additions, shapes and refusals.  fp32 in, fp32 out. */
int ld_dn_conv_f16(const ld_pc_conv_args* args, const void* weight_f16, void* stream);
int ld_dn_wgrad_f16(const float* dy, const float* a, float* work, float* dw, int B, int H, int W, int Cin, int Cout, int ksize,
                    int splits, void* stream);
int ld_dn_pack_conv_f16(const float* w_oihw, void* fwd_f16, void* dgr_f16, int co, int cop, int ci, int cip, int k, void* stream);

/* ---- device-resident training data (data.py's MNIST, MvtecDatasetSR and MedDataset_png as Trainer builds them): csrc/dataset.hip
 * One launch per batch: B rows of a device table choose B images of a device store and their augmentation; hr and lr come out as
 * contiguous fp32 NCHW, 16-byte aligned.  The rotation is torchvision's tensor rotate (NEAREST, expand = False, fill = None) about
 * the image centre, a positive angle counter-clockwise, followed by the vertical flip; (cos 1, sin 0, flip 0) is the identity
 * exactly.  Every operation is a single correctly rounded fp32 operation (IEEE division, nothing contracted), no floating-point
 * atomics, nothing allocates, nothing synchronises; a refused call returns LD_EINVAL before anything is launched.  The HOST
 * validates the table's indices against N (the kernels only clamp them). */
typedef struct ld_ds_row {
  int32_t src;             /* index of the image in the store, 0 <= src < N */
  float cos_a, sin_a;      /* of the rotation angle, computed in double and rounded */
  int32_t flip;            /* non-zero: reverse the rows after the rotation */
} ld_ds_row;
#define LD_DS_MIN_PARTS 16 /* row bands per image of ld_ds_mri_batch's minimum */
/* data.MNIST (data.py:814-836): store u8 [N, S, S] (S even; 28), hr / lr [B, 1, S, S].  hr = 2 (x / 255) of the transformed image;
 * lr = its even rows (all columns) brought back to S rows by bilinear interpolation (align_corners = False), then 2 (. / 255). */
int ld_ds_mnist_batch(const void* store_u8, int N, int S, const ld_ds_row* table, int B, float* hr, float* lr, void* stream);
/* MvtecDatasetSR (data.py:287-307, train, no denoise, no mask_train): store u8 [N, C, S, S], C 1 or 3, S even; hr / lr [B, C, S, S].
 * hr = (x / 255) 2; lr = the even rows and columns of hr (nearest to S / 2), bilinear back to S x S (align_corners = False):
 * columns first, then rows. */
int ld_ds_sr_batch(const void* store_u8, int N, int C, int S, const ld_ds_row* table, int B, float* hr, float* lr, void* stream);
/* MedDataset_png (data.py:369-442): two fp32 stores [N, R, R] of finite values; hr [B, 1, crop, crop] from target, lr from cond.
 * Centre crop (top = left = round((R - crop) / 2), half to even), the row's rotation and flip inside the crop for both (corners
 * fill with 0), (x - mean) / std with the modality's constants (std > 0), and with translate_zero + |min| of that image.  The
 * minimum takes a first launch that leaves LD_DS_MIN_PARTS partial minima per image in work (B * 2 * LD_DS_MIN_PARTS floats;
 * may be NULL without translate_zero).  crop a multiple of 4, crop <= R. */
int ld_ds_mri_batch(const float* target, const float* cond, int N, int R, int crop, const ld_ds_row* table, int B, float mean_target,
                    float std_target, float mean_cond, float std_cond, int translate_zero, float* work, float* hr, float* lr,
                    void* stream);
/* The two labelled data sets, for SegTrainer and MnistClassifierTrainer; the same table, rotation, flip and contract as above.
 * MedSegDataset (data.py:676-743) behind the .mha decode: image fp32 [N, R, R] of finite values, label_u8 [N, R, R]; x and target
 * fp32 [B, 1, crop, crop], 16-byte aligned.  ld_ds_mri_batch's centre crop, the row's rotation and flip inside the crop for both
 * (the reference has its flips commented out: (cos 1, sin 0, flip 0) is the reference); x = (v - mean) / std with v = 0 outside
 * the rotated image, target = label > 0 ? 1 : 0 and 0 outside.  One launch of B * 2 planes.  crop a multiple of 4, 4 <= crop <= R;
 * std positive and finite, mean a number. */
int ld_ds_seg_batch(const float* image, const void* label_u8, int N, int R, int crop, const ld_ds_row* table, int B, float mean,
                    float std, float* x, float* target, void* stream);
/* data.MNIST with its third return value (data.py:814-836): store u8 [N, S, S] (S even, 2..16384), labels_u8 [N]; x [B, 1, S, S]
 * is ld_ds_mnist_batch's hr (16-byte aligned; no lr is made), label [B] int64 (8-byte aligned), label[b] = labels_u8[src_b],
 * written by one thread per sample.  The HOST validates the labels' range; the kernel copies them. */
int ld_ds_mnist_cls_batch(const void* store_u8, const void* labels_u8, int N, int S, const ld_ds_row* table, int B, float* x,
                          long long* label, void* stream);

/* ---- quality metrics (metrics.hip): per-sample, per-region error sums for MSE / PSNR / SSIM ------------------------------ */
/* pred, ref fp32 NCHW [B, C, H, W] contiguous; mask [B, 1, H, W] fp32 or NULL.  out [B][3][4] fp64: region 0 = the whole image,
 * 1 = OOD (mask >= 1, ld_recompose's convention), 2 = IND (the rest; with mask NULL regions 1 and 2 are zeros); fields n_elem
 * (elements of the region over all channels), sse (d = pred - ref in fp32, widened, squared and added in double), n_win (SSIM
 * windows counted) and ssim_sum.  SSIM: Wang et al., 11 x 11 Gaussian window (sigma 1.5, the 11 taps computed in double and
 * rounded to fp32 once: ld_metric_taps), biased variances, K1 = 0.01, K2 = 0.03, C1 = (K1 L)^2 and C2 = (K2 L)^2 computed in double
 * and rounded once, L = data_range; only windows wholly inside the image count (no padding: (H - 10) x (W - 10) per channel), and
 * a window belongs to the region of its centre pixel.  Per window in fp32, no fused multiply-add: the five moments mu_x, mu_y,
 * E[x^2], E[y^2], E[xy] by a horizontal pass, then a vertical one, taps added in index order; sx = E[x^2] - mu_x^2, sy, sxy alike;
 * ssim = ((2 mu_x mu_y + C1)(2 sxy + C2)) / ((mu_x^2 + mu_y^2 + C1)(sx + sy + C2)) with IEEE division, widened to double.
 * Two launches: one workgroup per (sample, channel, 32 x 32 tile of window centres) leaves 12 partial sums in `work`
 * (ld_metric_work_doubles(B, C, H, W) doubles; 0 for a shape the call refuses), the second adds a sample's partial sums in
 * (channel, tile row, tile column) order.  No floating-point atomics: two calls give the same bits, and the result of sample b
 * depends neither on B nor on the other samples.  LD_EINVAL with nothing launched or written: a NULL pred, ref, work or out; B, C,
 * H or W below 1; H or W below 11; a data_range that is not finite and positive; out or work not 8-byte aligned (pred, ref,
 * mask: 4-byte); more than 2^31 - 1 tiles. */
int ld_metric_taps(float* taps /* host, 11 floats */);
int64_t ld_metric_work_doubles(int B, int C, int H, int W);
int ld_metric_sums(const float* pred, const float* ref, const float* mask, double* work, double* out, int B, int C, int H, int W,
                   float data_range, void* stream);

/* ---- the one collective of the path: all-gather of every rank's finished samples, RCCL over xGMI ---- */
/* RCCL is dlopen'ed on first use (the copy the process already mapped, e.g. torch's, is preferred; LD_RCCL_PATH
 * overrides), so the library loads without it.  ld_comm_unique_id on one rank -> hand the 128 bytes to every rank ->
 * ld_comm_init on each (uses the calling thread's current HIP device) -> ld_allgather enqueued on `stream`:
 * recv[r*bytes_per_rank ...] = rank r's send buffer -> ld_comm_destroy.  The product's default keeps this collective
 * in torch.distributed (same RCCL); dist.gather_patches uses these entry points when asked to. */
int ld_comm_unique_id(void* id_out_128 /* host, 128 bytes */);
int ld_comm_init(void** comm_out, const void* id_128 /* host */, int world, int rank);
/* The same with a deadline: the communicator comes up non-blocking (ncclCommInitRankConfig + ncclCommGetAsyncError polled
 * against timeout_s); if it is not up in time -- a peer that never arrives, a stale unique id -- it is aborted
 * (ncclCommAbort) and the call returns LD_ETIMEOUT instead of hanging.  timeout_s <= 0 = ld_comm_init (blocking).
 * ld_allgather / ld_comm_destroy on such a communicator poll with the same deadline where RCCL answers ncclInProgress. */
int ld_comm_init_timeout(void** comm_out, const void* id_128 /* host */, int world, int rank, double timeout_s);
int ld_allgather(const void* send, void* recv, size_t bytes_per_rank, void* comm, void* stream);
int ld_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* LOCALDIFF_HIP_H */
