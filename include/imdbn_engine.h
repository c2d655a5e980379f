/*
 * imdbn_engine.h -- C ABI of the MI355X (gfx950) contrastive-divergence engine.
 *
 * This is the drop-in boundary for the ONE hot path of francesco-cal98/multimodal-idbn
 * (SURVEY.md section 8).  The reference has no FFI: the path sits behind Python methods that
 * dispatch ATen ops.  Each entry point below replaces the ATen sequence of one reference
 * method (citations: file:line under /root/reference/imdbn/models/).  The Python classes in
 * multimodal-idbn_amd/imdbn/models/ keep the reference's signatures and call these through
 * ctypes (cffi, which BASELINE.json names, is not installed in the image).
 *
 * Conventions
 *   - extern "C", no exceptions cross the boundary; every function returns int:
 *       0 = ok, <0 = IMDBN_E_* below, >0 = hipError_t passed through.
 *     imdbn_last_error() returns the thread-local message of the last failure.
 *   - The caller (PyTorch) owns every buffer.  Pointers are raw DEVICE pointers
 *     (tensor.data_ptr()), fp32 row-major with an explicit leading dimension in ELEMENTS.
 *     The library allocates nothing persistent; scratch comes from the caller's workspace
 *     (imdbn_ws_bytes() tells how much; contents need not survive between calls).
 *   - Every launch goes to the hipStream_t passed in (torch.cuda.current_stream().cuda_stream);
 *     no call synchronises the host or touches another stream.  Graph-capturable.
 *   - Parameters are read through the descriptor at EVERY call -- the engine keeps no copy, so
 *     callers may mutate or re-bind W / biases between calls.
 *   - Randomness: imdbn_rng says where draws come from, in the reference's draw order
 *     (SURVEY.md Appendix B).  REPLAY consumes caller-recorded draws (parity tests);
 *     PHILOX generates Philox-4x32-10 keyed on (seed, draw number, GLOBAL row, column) so
 *     results do not depend on tiling or on data-parallel sharding.
 */
#ifndef IMDBN_ENGINE_H
#define IMDBN_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMDBN_ABI_VERSION 4

/* error codes (negative) */
#define IMDBN_E_INVALID   (-1)   /* bad argument (shape, null pointer, alignment) */
#define IMDBN_E_WORKSPACE (-2)   /* workspace too small */
#define IMDBN_E_RNG       (-3)   /* replay tape exhausted */
#define IMDBN_E_NODEVICE  (-4)   /* no gfx950 device */
#define IMDBN_E_UNSUPPORTED (-5)

/* arithmetic mode of the propagations / association products */
#define IMDBN_PARITY_F32 0   /* fp32 master weights split hi+mid+lo bf16 in registers: exact products */
#define IMDBN_FAST_BF16  1   /* one bf16 term per operand (throughput mode; not parity-grade) */

#define IMDBN_RNG_PHILOX 0
#define IMDBN_RNG_REPLAY 1

#define IMDBN_MAX_GROUPS 4

typedef void* imdbn_stream_t;    /* hipStream_t */

/* One RBM's parameters (rbm.py:41-79).  W is [V][ldw] with ldw >= H. */
typedef struct imdbn_rbm_desc {
    float*   W;
    int64_t  ldw;
    float*   hid_bias;      /* [H] */
    float*   vis_bias;      /* [V] */
    float*   W_m;           /* [V][ldw] momentum buffers; may be NULL for inference-only calls */
    float*   hb_m;          /* [H] */
    float*   vb_m;          /* [V] */
    int32_t  V, H;
    int32_t  mode;          /* IMDBN_PARITY_F32 | IMDBN_FAST_BF16 */
    int32_t  n_groups;      /* softmax groups over visible columns (rbm.py:66,113-114) */
    int32_t  group_start[IMDBN_MAX_GROUPS];
    int32_t  group_end[IMDBN_MAX_GROUPS];
} imdbn_rbm_desc;

/* Where random draws come from.  The *_used fields are OUTPUTS: how much the call consumed. */
typedef struct imdbn_rng {
    int32_t  mode;          /* IMDBN_RNG_PHILOX | IMDBN_RNG_REPLAY */
    int32_t  _pad;
    uint64_t seed;          /* PHILOX key */
    uint64_t offset;        /* PHILOX: number of the first draw tensor of this call */
    int64_t  row0;          /* PHILOX: global index of local row 0 (data-parallel shard offset) */
    const float*   tape;    /* REPLAY: device floats, uniform / normal draw tensors back to back */
    int64_t        tape_len;
    const int32_t* cat_tape;/* REPLAY: device int32, one index per (categorical draw, row) */
    int64_t        cat_len;
    int64_t  tape_used;     /* out */
    int64_t  cat_used;      /* out */
    uint64_t draws_used;    /* out: draw tensors consumed (advance `offset` by this) */
    const uint64_t* dev_offset; /* PHILOX, nullable: a device-resident counter the kernels ADD to `offset` when they run.  A call
                               sequence captured into a hipGraph bakes `offset` in; with dev_offset set and an
                               imdbn_rng_advance(dev_offset, draws_used, stream) node behind it, every replay of the graph draws
                               fresh numbers -- exactly those the same calls would draw issued one by one. */
} imdbn_rng;

/* One half-step pair v -> h -> v' of a conditional chain
 * (rbm.py:275-291 annealed Gibbs, :337-365 noisy mean-field, :393-399 plain Gibbs). */
typedef struct imdbn_chain_step {
    float   T;              /* temperature of both half steps (max(1e-6,T) applied by callee) */
    float   sigma;          /* std of Gaussian noise added to both logits; 0 = none, no draw */
    float   eta;            /* mu-pull weight on columns [0,Dz) (rbm.py:359-363); 0 = off */
    int32_t sample_h;       /* 1: h = 1[p_h > U] ; 0: h = p_h */
    int32_t vmode;          /* 0: v = p_v ; 1: v = sampleV(p_v) ; 2: v = sampleV(mix(p_v)) w/o re-mix */
    int32_t clamp;          /* 1: v = v*(1-mask) + v_known*mask (masks must be 0/1) */
} imdbn_chain_step;

enum { IMDBN_DATA_UNKNOWN = 0, IMDBN_DATA_BINARY = 1, IMDBN_DATA_REAL = 2 };      /* imdbn_cd_opts.data_binary / next_binary */

/* Options of one CD update (rbm.py:181-227, :403-483). */
typedef struct imdbn_cd_opts {
    int32_t cd_k;           /* Gibbs steps of the negative phase (>=1) */
    float   lr;             /* effective learning rate: lr/(1+0.01*epoch) [* aux_lr_mult] (rbm.py:194,476) */
    float   momentum;       /* momentum or final_momentum (rbm.py:195) */
    float   weight_decay;
    int32_t sparsity;       /* rbm.py:217-219 (train_epoch only) */
    float   sparsity_target;
    int32_t sample_h;       /* clamped step only (rbm.py:462) */
    int32_t sample_v;       /* clamped step only (rbm.py:468) */
    int32_t reclamp_negative; /* clamped step only (rbm.py:464) */
    /* -- next-batch prefetch (imdbn_rbm_cd_step only; all zero = off).  The operand forms of a batch are a pure
     * function of the batch: cd_step can prepare those of the FOLLOWING batch with extra blocks of its first
     * negative-phase launch, into prefetch slot 1 or 2 of the workspace, and a later cd_step on the same workspace is told that
     * its `data` already sits in that slot.  The caller guarantees the batch was not modified in between. */
    const float* next_data; /* [B][V] fp32 batch to prepare during this call (NULL: none); honoured only when
                               imdbn_rbm_prefetch_ok() says so for this descriptor and batch size */
    int64_t ld_next;
    int32_t next_slot;      /* 1 or 2: where to put it (must differ from data_slot) */
    int32_t data_slot;      /* 0: prepare `data` now (default); 1 / 2: `data` was prefetched into that slot */
    /* -- what the caller knows about the VALUES of `data` (IMDBN_DATA_*).  Nothing has to be known: with IMDBN_DATA_UNKNOWN (0)
     * the device decides, per 64-column piece of the batch and from the exactness map its own preparation kernel writes, whether the
     * positive phase reads that piece as a bit plane (all values 0 / 1: binary images) or as bf16 terms; the result is the same
     * number either way, so the caller never has to inspect a batch (no device reduction, no host synchronisation).
     * IMDBN_DATA_BINARY (1): the caller asserts every element is exactly 0 or 1; the assertion is checked on the device and a
     * batch that is not binary turns the update into NaN instead of being silently truncated.  IMDBN_DATA_REAL (2): real values
     * (the output of another layer): no bit plane is made. */
    int32_t data_binary;
    /* -- the same for `next_data`.  UNKNOWN: every 64-column x 64-row piece that turns out to be all 0 / 1 is prepared in the slim
     * form (bit plane, exactness map, column sums, one bf16 plane), any other piece with all three-term operand forms; BINARY: the
     * slim form throughout.  Honoured where the positive phase can read bit planes (16-B aligned weight rows, V > 1024); the later
     * cd_step on that batch must pass the same value in data_binary. */
    int32_t next_binary;
    /* -- forward pass fused behind the update (imdbn_rbm_cd_step only; NULL = off): after the weights are updated, the
     * hidden probabilities sigmoid(data @ W + hid_bias) of the SAME batch under the NEW weights are written to
     * fwd_out[B][H] (row stride ld_fwd floats) -- the `train_epoch(v); v = forward(v)` pair of the layer loop
     * (idbn.py:195-204) as one call: the batch's operand forms are still in the workspace, so nothing is prepared twice. */
    float*  fwd_out;
    int64_t ld_fwd;
} imdbn_cd_opts;

/* ---- plumbing ------------------------------------------------------------------------- */
int    imdbn_version(void);
int    imdbn_last_error(char* buf, size_t n);
/* cu_count / arch name of the current device; IMDBN_E_NODEVICE without a GPU */
int    imdbn_device_info(int* cu_count, char* arch, size_t n);
/* bytes of scratch any call below needs for an RBM of V x H at batch B */
size_t imdbn_ws_bytes(int V, int H, int B);
/* tuning knobs (split-K factors); 0 = automatic */
int    imdbn_set_tuning(int ksplit_up, int ksplit_down);
/* named tuning/testing knobs (process-wide defaults).  Tuning (0 = automatic): "ksplit_up", "ksplit_down", "k1s_ks",
 * "down_rows" (0 or a multiple of 4 in [4, 32]), "k2s_rows" (0 or a multiple of 8 in [8, 48]), "chain_rows" ([0, 16]),
 * "min_rank_loop".  Testing, 1 = take the other kernel path: "generic_k3" (the unaligned-shape K3), "generic_k1",
 * "no_fused_up", "no_k1s", "no_k1s_real", "no_k2s", "no_bits", "no_prefetch", "no_adaptive", "no_chain_kernel",
 * "no_chain_pair", "no_down_chunks", "no_down_tiled", "no_rank_loop", "no_rank_acc", "no_update_bin"
 * (0/1 batches update through assoc_update_planes, not the two-plane kernel), "k3_tpb" (visible tiles per block of the streaming
 * update kernels, clamped to [0, 64]; 0 = automatic).  Experiments: "k1s_lds_pad" (bytes,
 * clamped to [0, 65536]), "k1s_force_na".  Process-wide only: "dbg" (timeline stamps).  None of them changes results
 * beyond fp32 summation order, none is needed for normal use */
int    imdbn_set_option(const char* name, int value);
/* The same knobs per caller instead of per process: a handle starts as a copy of the process defaults, takes
 * imdbn_options_set(name, value) (every name of imdbn_set_option but "dbg"), and imdbn_use_options(handle) binds it to the
 * CALLING THREAD: engine calls made by that thread read the handle (NULL = back to the process defaults).  Knobs that shape
 * the workspace layout (split-K factors, tile heights) must agree between calls that share a workspace. */
typedef struct imdbn_options imdbn_options;
imdbn_options* imdbn_options_create(void);
void   imdbn_options_destroy(imdbn_options* o);
int    imdbn_options_set(imdbn_options* o, const char* name, int value);
int    imdbn_use_options(const imdbn_options* o);
/* per-kernel timing of the update kernel with HIP events on the launch stream (bench.py roofline) */
int    imdbn_profile_enable(int on);
int    imdbn_profile_read(double* total_ms, int* launches);   /* synchronises the recorded events */
/* tuning aid: copies the per-block wall-clock stamps (100 MHz ticks, 8 per block, up to 4096 blocks) that the
 * propagation kernels record when the "dbg" option enables them; synchronises the device */
int    imdbn_debug_stamps(long long* out, int n);
/* test / tuning aid: byte offset of a named internal buffer inside the workspace of an (V, H, B) call ("vis_bits0/1", "hid_bits",
 * "vis_tr0/1", "hid_tr0/1", "cs_hpos/hneg/vpos/vneg", "flags", "partial", "vis_rm1", and of the prefetch slots 1 / 2 "pf_tr1/2",
 * "pf_bits1/2"); the layout is NOT part of the ABI */
int    imdbn_debug_ws_offset(int V, int H, int B, const char* name, size_t* offset);
/* test aid: which kernel family the last up (v -> h) and the last down (h -> v) propagation of the CALLING THREAD launched,
 * recorded by the launchers where they launch (host code only; the routes themselves are NOT part of the ABI).
 * route[0] = up family (IMDBN_ROUTE_UP_*), route[1] = 1 if that launch ran the general epilogue, 0 the lean one;
 * route[2] = down family (IMDBN_ROUTE_DOWN_*), route[3] = its epilogue likewise, route[4] = 1 if the softmax-group kernel
 * (finish_groups) followed it.  A family is -1 until the thread has run such a propagation.  The row-parallel chain kernel,
 * the CD update kernel and every call that runs no propagation leave the record as it was. */
enum { IMDBN_ROUTE_UP_FUSED = 0, IMDBN_ROUTE_UP_STREAM_BITS = 1, IMDBN_ROUTE_UP_STREAM_REAL = 2, IMDBN_ROUTE_UP_PARTIAL4 = 3,
       IMDBN_ROUTE_UP_PARTIAL = 4 };
enum { IMDBN_ROUTE_DOWN_K2_STREAM = 0, IMDBN_ROUTE_DOWN_FUSED = 1, IMDBN_ROUTE_DOWN_CHUNKS2 = 2, IMDBN_ROUTE_DOWN_CHUNKS4 = 3,
       IMDBN_ROUTE_DOWN_TILED = 4 };
int    imdbn_debug_last_route(int route[5]);
/* test aid, likewise for the weight update: rec[0] = the kernel the last update of the CALLING THREAD launched (IMDBN_UPDATE_*; the
 * last launch of a multi-chunk batch; -1 until the thread has run an update), rec[1] = visible tiles per block of that launch
 * (0 for the generic kernel).  Host code only; the routes are NOT part of the ABI */
enum { IMDBN_UPDATE_GENERIC = 0, IMDBN_UPDATE_PLANES = 1, IMDBN_UPDATE_BIN = 2, IMDBN_UPDATE_RANKS = 3 };
int    imdbn_debug_last_update(int rec[2]);
/* test aid, likewise for the chains (imdbn_rbm_chain*, the positive phase of imdbn_rbm_clamped_*): rec[0] = how the last chain of the
 * CALLING THREAD ran (IMDBN_CHAIN_*: one launch per half step, the row-parallel chain kernel, or that kernel running both chains of
 * a pair in one launch; -1 until the thread has run a chain), rec[1] = batch rows per block of the kernel launch, rec[2] = its
 * blocks (both 0 for IMDBN_CHAIN_PER_LAUNCH), rec[3] = the records of chain 0 (its steps plus a traced baseline).  A pair that does
 * not run as one launch reports its second chain's run.  Host code only; the routes are NOT part of the ABI */
enum { IMDBN_CHAIN_PER_LAUNCH = 0, IMDBN_CHAIN_KERNEL = 1, IMDBN_CHAIN_KERNEL_PAIR = 2 };
int    imdbn_debug_last_chain(int rec[4]);
/* test aid, likewise for the CD pass (imdbn_rbm_cd_step / _cd_stats / _cd_factors / _cd_factors_wire, and the CD pass of the calls
 * built on it), whose first launches imdbn_debug_last_route no longer shows at the end of the call: rec[0] = the up family of the
 * positive-phase K1 of the last CD pass of the CALLING THREAD, rec[1] = the down family of its first K2, rec[2] = the up family of
 * its last K1 (IMDBN_ROUTE_*; -1 until the thread has run a CD pass), rec[3] = where the next batch (imdbn_cd_opts.next_data) was
 * prepared (IMDBN_CD_NEXT_*: not at all -- no hint, or the route ignores it --, by a prep_operand launch of its own, by extra blocks
 * of the fused K2, by extra blocks of the negative-phase k1_stream), rec[4] = the prefetch slot the data were read from
 * (imdbn_cd_opts.data_slot, 0 = none), rec[5] = 1 if that preparation decided the forms per 64-column item (a batch of unknown
 * content).  Host code only; the routes are NOT part of the ABI */
enum { IMDBN_CD_NEXT_NONE = 0, IMDBN_CD_NEXT_OWN_LAUNCH = 1, IMDBN_CD_NEXT_FUSED_K2 = 2, IMDBN_CD_NEXT_K1_STREAM = 3 };
int    imdbn_debug_last_cd(int rec[6]);

/* *dev_offset += n on `stream` (see imdbn_rng.dev_offset).  Every engine call is a plain sequence of kernel launches on the caller's
 * stream -- no host synchronisation, no allocation, no memcpy -- so it can be recorded with hipStreamBeginCapture. */
int imdbn_rng_advance(uint64_t* dev_offset, uint64_t n, imdbn_stream_t stream);

/* ---- K1: p(h|v)   replaces RBM.forward (rbm.py:81-92) ---------------------------------- */
/* out_prob[B][H] = sigmoid((v W + c)/T);  out_sample (nullable) = 1[out_prob > U] */
int imdbn_rbm_prop_up(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, float T,
                      imdbn_rng* rng, float* out_prob, int64_t ldo, float* out_sample, int64_t lds,
                      void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* forward(v) at T = 1: out_prob[B][H] = sigmoid(v W + c).  data_binary = IMDBN_DATA_* as in imdbn_cd_opts (UNKNOWN: the device
 * reads every 64-column piece of v as a bit plane or as bf16 terms, whichever describes it; BINARY: asserted, checked, NaN on a
 * false promise).  Bit-identical to the fused forward of imdbn_rbm_cd_step (imdbn_cd_opts.fwd_out) for the same batch and
 * weights, whatever data_binary says. */
int imdbn_rbm_forward(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, int data_binary,
                      float* out_prob, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- free energy   F(v) = -v.b - sum_j softplus(c_j + (vW)_j)   (imdbn/utils/energy_utils.py:19-28; the
 *      `joint_rbm.free_energy` that imdbn.py:455-474 probes for and the reference never defines) -------- */
int imdbn_rbm_free_energy(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B, float* out_F,
                          void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- annealed importance sampling (imdbn/utils/likelihood.py; Salakhutdinov & Murray 2008) ----------------------------------------
 * M independent chains from the base-rate model A (W = 0, hidden biases 0, visible biases base_vis_bias; NULL = zeros) to the RBM
 * through the temperatures 0 = betas[0] < betas[1] < ... < betas[K] = 1 (HOST array of K + 1 floats), x(v) = hid_bias + v W,
 * sp = softplus in double:
 *   v_1 = 1[sigmoid(b_A) > U];  for k = 1..K:
 *     logw += (beta_k - beta_{k-1}) sum_i (b_i - b_A,i) v_i + sum_j [sp(beta_k x_j) - sp(beta_{k-1} x_j)]     (both sums in double)
 *     k < K:  h = 1[sigmoid(beta_k x) > U];  v_{k+1} = 1[sigmoid(beta_k (b + h W^T) + (1 - beta_k) b_A) > U]
 *   logw[M] (device, double) is OVERWRITTEN with the log importance weights; log Z ~= H log 2 + sum_i sp(b_A,i) + logmeanexp(logw).
 *   out_v (nullable): the final state v_K [M][V], row stride ldo >= V.
 * Draws: ("u", V), then K - 1 times ("u", H), ("u", V): draws_used = 2 K - 1.  Both sums of logw run in an order fixed by (V, H),
 * the logits are those of the propagations, and Philox is keyed on the row: chain i is the same chain whatever M (bit for bit
 * while M stays within the same multiple of 64 rows); no floating-point atomics.
 * IMDBN_E_INVALID (naming the value): M < 1, K < 1, betas[0] != 0, betas[K] != 1, betas not increasing, null betas / rng / logw;
 * IMDBN_E_UNSUPPORTED: softmax groups.  Nothing is launched and logw is untouched on any error.
 * Workspace: imdbn_ws_bytes(V, H, M).  The caller's parameters are only read. */
int imdbn_rbm_ais(const imdbn_rbm_desc* d, int M, int K, const float* betas, const float* base_vis_bias, imdbn_rng* rng,
                  double* logw, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- AIS over Bernoulli visibles plus softmax groups (imdbn/utils/likelihood.py: estimate_joint_log_partition) ----
 * imdbn_rbm_ais for 0 <= n_groups <= IMDBN_MAX_GROUPS: same arguments, same checks (naming the value; logw untouched on any error).
 * Inside a group the columns of base_vis_bias are the logits of a categorical, so
 *   log Z_A = H log 2 + sum_{i not in a group} sp(b_A,i) + sum_g logsumexp(b_A[g]).
 *   v_1: Bernoulli columns as imdbn_rbm_ais; each group one category from softmax(b_A[g]).
 *   The weight increment is the formula of imdbn_rbm_ais on the one-hot state.
 *   v_{k+1}: the sampling down propagation at T = 1 / beta_k with the bias b + ((1 - beta_k) / beta_k) b_A; a group is drawn from
 *   softmax(beta_k (b + h W^T) + (1 - beta_k) b_A).  Every categorical is the draw of the softmax-group kernel of the propagations:
 *   fp32 softmax, inverse CDF over clamp(p, 1e-8, 1) in column order (PHILOX), or the index on cat_tape (REPLAY).
 * Draws: ("u", V), ("c", w_g) per group, then K - 1 times ("u", H), ("u", V), ("c", w_g) per group:
 * draws_used = (K - 1) (2 + G) + 1 + G.  With n_groups = 0 the call is imdbn_rbm_ais bit for bit.
 * Workspace: imdbn_ws_bytes(V, H, M).  The caller's parameters are only read. */
int imdbn_rbm_ais_groups(const imdbn_rbm_desc* d, int M, int K, const float* betas, const float* base_vis_bias, imdbn_rng* rng,
                         double* logw, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- reverse annealed importance sampling (imdbn/utils/likelihood.py: reverse_ais_log_likelihood; Burda, Grosse & Salakhutdinov
 *      2015) ---------------------------------------------------------------------------------------------------
 * The forward AIS chain read as a generative model p_ann (v_1 ~ p_A, v_{k+1} ~ T_k(. | v_k) for k = 1..K, T_k the transition of
 * imdbn_rbm_ais_groups at beta_k, one transition at beta_K = 1 included; the sample is v_{K+1}), run backwards from the start states
 * v [R][V] (0/1, row stride ldv; the caller replicates a test row once per chain).  With Delta_k the increment of imdbn_rbm_ais:
 *   logw = sum_i b_i v_i + sum_j sp(x_j(v))                                     (= -F(v))
 *   for k = K..1:  u_k ~ T_k(. | u_{k+1});  logw -= Delta_k(u_k)                 (u_{K+1} = v)
 * logw[R] (device, double) is OVERWRITTEN; exp(logw) / Z_A is an unbiased estimate of p_ann(v), log Z_A as imdbn_rbm_ais_groups
 * defines it (NOT included).  out_v (nullable): the final state u_1 [R][V], row stride ldo >= V.  0 <= n_groups <= IMDBN_MAX_GROUPS.
 * A row holding an element that is not exactly 0 or 1, or a softmax group without exactly one 1, gets logw = NaN, that row only
 * (checked on the device).
 * Draws: K times ("u", H), ("u", V), ("c", w_g) per group: draws_used = K (2 + G).  Sums, logits and the Philox key as in
 * imdbn_rbm_ais: row i is the same chain whatever R (bit for bit while R stays within the same multiple of 64 rows).
 * IMDBN_E_INVALID (naming the value): R < 1, K < 1, betas[0] != 0, betas[K] != 1, betas not increasing, null v / betas / rng / logw,
 * ldv < V, ldo < V.  Nothing is launched and logw is untouched on any error.
 * Workspace: imdbn_ws_bytes(V, H, R).  The caller's parameters are only read. */
int imdbn_rbm_reverse_ais(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int R, int K, const float* betas,
                          const float* base_vis_bias, imdbn_rng* rng, double* logw, float* out_v, int64_t ldo,
                          void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* Row n owns logw[n M .. n M + M - 1] (device, double): out_lme[n] = log((1 / M) sum_m exp(logw)), out_ess[n] = (sum w)^2 / sum w^2 on
 * the weights shifted by the row's maximum; both double [N], summed in an order fixed by M.  A NaN makes both outputs of its row NaN
 * and no other.  IMDBN_E_INVALID: N < 1, M < 1, a null pointer. */
int imdbn_rows_logmeanexp(const double* logw, int N, int M, double* out_lme, double* out_ess, imdbn_stream_t stream);

/* ---- label side of the joint RBM's log-likelihood (imdbn/utils/likelihood.py: imdbn_sample_values) -------------
 * d: the joint RBM, labels in the visible columns [Dz, Dz + K).  For every row of z [N][Dz] (fp32, 0/1 or real, row stride ldz), with
 * base = hid_bias + z W[:Dz] (one up propagation on the first Dz weight rows) and a_k = z . b_z + b_{Dz+k} + sum_j sp(base_j + W[Dz+k][j]):
 *   out_joint[row] = a_{gt[row]}          = -F([z, e_gt])               (NaN when gt[row] is outside [0, K); nothing is read through it)
 *   out_marg[row]  = logsumexp_k a_k      = log sum_y exp(-F([z, y]))
 * both in double (device, [N]), every sum in an order fixed by (Dz, K, H): a row gives the same bits alone and inside a batch.
 * IMDBN_E_INVALID (naming the value) before the first launch: K outside [2, 256], Dz < 1, Dz + K > V, N < 1, ldz < Dz, a null
 * pointer.  Workspace: imdbn_ws_bytes(Dz, H, N).  No draws.  The caller's parameters are only read. */
int imdbn_rbm_label_loglik(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                           double* out_joint, double* out_marg, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- one ascent step on log p(y | z) of the joint RBM (imdbn/models/rbm.py: train_epoch_labels) ------------------
 * d: the joint RBM with its momentum buffers, visible = [code (Dz) | labels (K)], Dz + K == V.  No reference counterpart (its w_sup is
 * unused); the exact gradient of the hybrid objective of Larochelle & Bengio (2008).  With base and a_k as above, U = W[Dz:],
 * o_kj = base_j + U_kj, s = sigmoid(o), t = gt[row]:
 *   out_logp[row] = a_t - logsumexp_k a_k       double [N]; the bits of out_joint - out_marg of imdbn_rbm_label_loglik on the parameters
 *                                               on entry; NaN when t is outside [0, K)
 *   p_k = exp(a_k - logsumexp a),  r_k = 1[k = t] - p_k,  hpos_j = s_tj,  hneg_j = sum_k p_k s_kj
 *   G_W[:Dz] = z^T hpos - z^T hneg,  G_W[Dz + k][j] = sum_n r_nk s_nkj,  G_c = sum_n (hpos - hneg),  G_b[Dz + k] = sum_n r_nk,  G_b[:Dz] = 0
 * and the update of imdbn_rbm_cd_step (rbm.py:212-224) with (pos - neg) replaced by G, the divisor N and no sparsity term, on every
 * parameter:  W_m = momentum W_m + lr (G_W / N - weight_decay W), W += W_m;  hb_m = momentum hb_m + lr G_c / N, hid_bias += hb_m;
 * vb_m = momentum vb_m + lr G_b / N, vis_bias += vb_m (the code columns get their momentum only).  Of o only lr, momentum and
 * weight_decay are read.  All gradients come from the parameters on entry.  A row whose label is outside [0, K) enters no sum (the
 * divisor stays N) and nothing is read through its label.
 * The class values are summed in double as in imdbn_rbm_label_loglik; s, p_k and r_k are fp32, hneg and the sums over n of the label
 * side are single fp32 fma chains in index order, the code side runs the update kernel's exact products: every sum has an order fixed
 * by (Dz, K, H, N), no floating-point atomics, the same call on the same state gives the same bits.
 * scratch: N (K + 2 H) floats of the caller's (device; r, hpos, hneg between the launches; contents on return unspecified).  The
 * workspace is that of the propagation on the first Dz weight rows, which has no room sized by K.
 * IMDBN_E_INVALID (naming the value) before the first launch, no parameter and no output touched: a null momentum buffer, K outside
 * [2, 256], Dz < 1, Dz + K != V, N < 1, ldz < Dz, a null z / gt / o / out_logp / scratch.  Workspace: imdbn_ws_bytes(Dz, H, N).
 * No draws, no host synchronisation, plain launches on `stream`. */
int imdbn_rbm_label_step(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                         const imdbn_cd_opts* o, double* out_logp, float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- log p(y | z) of the joint RBM as an output layer: its error at the code z (imdbn/models/imdbn.py: discriminative_step; DESIGN
 * section 27) ----
 * d, z, gt, base, a_k, s, p_k, hpos, hneg as in imdbn_rbm_label_step.  From the parameters on entry:
 *   out_logp[row]  the bits of imdbn_rbm_label_step / imdbn_rbm_label_loglik (joint - marginal); NaN when t is outside [0, K)
 *   out_pred[row]  (nullable) argmax_k a_k over the double class values of the same row pass, the lowest k on a tie; written for every
 *                  row whatever gt holds (-1 only where every class value is NaN)
 *   e_j = hpos_j - hneg_j                     fp32 [N][H], one subtraction
 *   g_z = e W[:Dz]^T                          = d log p(t | z) / d z  (the visible biases of the code cancel)
 *   err_z = g_z z (1 - z)                     [N][Dz], row stride lde: the ascent direction at the pre-activations that produced z, the
 *                                             e_h imdbn_rbm_backprop_step expects for the layer whose output z is
 * A row whose label is outside [0, K) gets logp = NaN and an exact zero row of err_z; nothing is read through its label.  g_z is the
 * logits-only down propagation of imdbn_rbm_backprop_step's err_v_out on the descriptor cut to its first Dz weight rows, without a
 * bias (a signed real operand, whatever kernel route that shape takes), the product with z (1 - z) one fp32 multiplication.
 * o != NULL: also the update of imdbn_rbm_label_step; the six parameter and momentum tensors after the call are bit for bit those of
 * imdbn_rbm_label_step on the same state (lr, momentum, weight_decay are read; cd_k, sparsity, the prefetch fields and fwd_out must be
 * zero).  o == NULL: the head is frozen, no parameter is written and the momentum pointers may be null.
 * Launch order (plain launches on `stream`): the propagation of base; the row kernel (logp, pred, r, hpos, hneg, e); with o the
 * label-row update (it writes W[Dz:] and the label biases only, and is the last reader of base); the propagation of e through W[:Dz]
 * and the z (1 - z) epilogue (they read W[:Dz] only); with o the code-side update (the only writer of W[:Dz] and hid_bias), last.
 * Every order is fixed by (Dz, K, H, N); no floating-point atomics, no draws; the same call on the same state gives the same bits.
 * scratch: N (K + 3 H) floats of the caller's (device; r, hpos, hneg, e between the launches; contents on return unspecified).
 * IMDBN_E_INVALID (naming the value) before the first launch, no parameter and no output touched: the cases of
 * imdbn_rbm_label_step (a null o excepted), a null err_z, lde < Dz; with o a null momentum buffer or a non-zero cd_k, sparsity,
 * prefetch field or fwd_out.  Workspace: imdbn_ws_bytes(Dz, H, N).  No host synchronisation. */
int imdbn_rbm_label_backprop_step(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, const int32_t* gt,
                                  const imdbn_cd_opts* o, double* out_logp, int32_t* out_pred, float* err_z, int64_t lde,
                                  float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- exact pseudo-log-likelihood (imdbn/utils/likelihood.py: pseudo_log_likelihood) -----------------------------
 * PLL(v) = sum over sites of log p(v_site | v_rest), a site being every visible column outside the softmax groups and every group
 * as a whole.  No reference counterpart; built over the free energy above: with x = hid_bias + v W, sigma = sigmoid(x), s_i = 1 - 2 v_i,
 *   Bernoulli column i:  g_i = s_i b_i + sum_j log1p(sigma_j expm1(s_i W_ij)) = F(v) - F(v with bit i flipped);   term = -softplus(g_i)
 *   group, observed t:   g_k = (b_k - b_t) + sum_j log1p(sigma_j expm1(W_kj - W_tj));   term = -log sum_{k in group} exp(g_k)
 *   out_pll[N] (device, double) = the sum of the row's terms.
 *   out_site[N][V] (nullable, fp32, row stride lds): the term of column i; a group's term sits at its observed column and the
 *   group's other columns hold 0, so a row of out_site sums to out_pll.
 * v [N][V] is 0/1 with one-hot groups, row stride ldv; 0 <= n_groups <= IMDBN_MAX_GROUPS.  A row holding an element that is not
 * exactly 0 or 1, or a group without exactly one 1, gets out_pll = NaN and a NaN row in out_site, that row only (checked on the
 * device).  The logits are those of the propagations; the j sums run in fp32 over chunks of 128 hidden units and in double across
 * the chunks, every other sum in double, all in an order fixed by (V, H, groups): a row gives the same bits alone and inside any
 * batch; no floating-point atomics.  No draws.
 * IMDBN_E_INVALID (naming the value): N < 1, null v / out_pll, ldv < V, out_site with lds < V.  Nothing is launched and no output
 * is touched on any error.  Workspace: imdbn_ws_bytes(V, H, N).  The caller's parameters are only read. */
int imdbn_rbm_pseudo_loglik(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int N, double* out_pll, float* out_site, int64_t lds,
                            void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- one directed layer of the DBN lower bound (imdbn/utils/likelihood.py: dbn_sample_values; the same paper, §4) -----------------
 * For every row of v [M][V] (0/1 or real in [0, 1], row stride ldv), x = hid_bias + v W, sp = softplus in double:
 *   h = 1[sigmoid(x) > U]                         -> out_h [M][H] fp32 0/1, row stride ldh (the decision of imdbn_rbm_prop_up's sample)
 *   a = vis_bias + h W^T
 *   acc[row] += sum_i (v_i a_i - sp(a_i)) + E     log p(v | h) under the directed layer, plus
 *     IMDBN_BOUND_ENTROPY  E = sum_j (sp(x_j) - x_j sigmoid(x_j))     the entropy of q(h | v)
 *     IMDBN_BOUND_LOGQ     E = -sum_j (h_j x_j - sp(x_j))             -log q(h | v) of the drawn h
 *   acc[M] (device, double) is only ADDED to (the caller zeroes it); the two additions are two launches of one stream.
 * Draws: ("u", H): draws_used = 1.  Every sum runs in an order fixed by (V, H), the logits are those of the propagations, and
 * Philox is keyed on the row: row i is the same whatever M; no floating-point atomics.
 * IMDBN_E_INVALID (naming the value): M < 1, unknown mode, null v / rng / acc / out_h, ldv < V, ldh < H; IMDBN_E_UNSUPPORTED:
 * softmax groups.  Nothing is launched and acc is untouched on any error.
 * Workspace: imdbn_ws_bytes(V, H, M).  The caller's parameters are only read. */
#define IMDBN_BOUND_ENTROPY 0
#define IMDBN_BOUND_LOGQ    1
int imdbn_rbm_bound_step(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int M, int mode, imdbn_rng* rng,
                         double* acc, float* out_h, int64_t ldh, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- K2: p(v|h)  replaces RBM.visible_probs / backward (rbm.py:94-116,137-151) -------- */
/* out_prob[B][V] = sigmoid((h W^T + b)/T) with softmax over each group; if logits_only: raw logits */
int imdbn_rbm_prop_down(const imdbn_rbm_desc* d, const float* h, int64_t ldh, int B, float T,
                        int logits_only, float* out_prob, int64_t ldo,
                        void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- sample_visible (rbm.py:118-135) ---------------------------------------------------- */
int imdbn_rbm_sample_visible(const imdbn_rbm_desc* d, const float* v_prob, int64_t ldp, int B,
                             imdbn_rng* rng, float* out, int64_t ldo, imdbn_stream_t stream);

/* ---- one Gibbs step (rbm.py:158-178): outputs v_next, v_prob, h, h_prob ------------------ */
int imdbn_rbm_gibbs_step(const imdbn_rbm_desc* d, const float* v, int64_t ldv, int B,
                         int sample_h, int sample_v, imdbn_rng* rng,
                         float* v_next, float* v_prob, float* h, float* h_prob,
                         void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- whole RBM.train_epoch (rbm.py:180-227): K1 -> [K2 -> K1]^k -> K3 -> bias/loss -------- */
/* loss_out: device float[1] = mean((data - v_prob)^2) */
int imdbn_rbm_cd_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B,
                      const imdbn_cd_opts* o, imdbn_rng* rng, float* loss_out,
                      void* ws, size_t ws_bytes, imdbn_stream_t stream);
/* 1 when cd_step on this descriptor / batch size honours imdbn_cd_opts.next_data (16-B aligned weight rows: the
 * float4 fused K2 carries the prefetch blocks), else 0 -- then next_data is ignored and nothing may be assumed prefetched. */
int imdbn_rbm_prefetch_ok(const imdbn_rbm_desc* d, int B);

/* ---- persistent contrastive divergence (imdbn/models/rbm.py: train_epoch_persistent; Tieleman 2008) -------------
 * The update of imdbn_rbm_cd_step (rbm.py:199-226) with the negative phase taken from caller-owned chains instead of from the data.
 * particles [B][V]: fp32, 0/1, one-hot inside softmax groups, row stride ldp >= V; READ AND OVERWRITTEN.
 *   pos_h = sigmoid(data W + c);   pos_assoc = data^T pos_h
 *   v = particles;  o->cd_k times (cd_k >= 0; 0: the particles as they are):
 *       h = 1[sigmoid(v W + c) > U];   v = sample_visible(visible_probs(h))              ("u", H), ("u", V), ("c", w_g) per group
 *   h_neg = sigmoid(v W + c) (probabilities, no draw);   neg_assoc = v^T h_neg
 *   the update of rbm.py:212-224 with (h_prob, v) := (h_neg, v), divisor B, the sparsity term from pos_h when o->sparsity
 *   particles := v
 * draws_used = cd_k (2 + G); rng may be NULL when cd_k = 0.
 * loss_out (device float[1], nullable): mean((data - v_rec)^2) with v_rec = visible_probs(pos_h) at T = 1, the mean-field
 * reconstruction error -- one more down propagation (a persistent chain does not reconstruct the batch, so the v_prob of
 * imdbn_rbm_cd_step does not exist here); NULL: that propagation is not launched.
 * o->data_binary as in imdbn_rbm_cd_step; the prefetch fields (next_data, next_slot, data_slot, next_binary) and fwd_out must be zero.
 * Every sum has the order imdbn_rbm_cd_step gives it; the same call on the same state gives the same bits.
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: a null momentum buffer, null data / particles / o,
 * ldd < V, ldp < V, B < 1, cd_k < 0, a null rng with cd_k > 0, a non-zero prefetch field or fwd_out; IMDBN_E_RNG: a replay tape
 * shorter than the draws.  Workspace: imdbn_ws_bytes(V, H, B); the reconstruction needs no more. */
int imdbn_rbm_pcd_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, float* particles, int64_t ldp,
                       const imdbn_cd_opts* o, imdbn_rng* rng, float* loss_out, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- centered update: the centering trick / enhanced gradient (imdbn/models/rbm.py: train_epoch_centered; Montavon & Mueller 2012;
 * Cho, Raiko & Ilin 2011; Melchior, Fischer & Wiskott 2016) -------------------------------------------------------
 * A centered RBM with offsets mu (visible) and lam (hidden) is the normal RBM with the biases b - W lam and c - W^T mu: the NORMAL
 * parameters stay stored and only the gradient changes.  mu [V], lam [H]: device fp32, READ AND OVERWRITTEN.
 * Phases, unchanged: particles == NULL: those of imdbn_rbm_cd_step (cd_k >= 1; draws ("u", H), then cd_k times ("u", V), ("c", w_g)
 * per group, ("u", H): draws_used = 1 + cd_k (2 + G)); loss = mean((data - v_prob)^2).  particles != NULL ([B][V], row stride
 * ldp >= V, advanced IN PLACE): those of imdbn_rbm_pcd_step (cd_k >= 0, draws_used = cd_k (2 + G), rng may be NULL when cd_k = 0);
 * loss = the mean-field reconstruction error, and with loss_out == NULL that propagation is not launched.  loss_out is nullable
 * in both cases.  With n = B, the column sums sv+ / sv- / sh+ / sh- of the positive / negative visible and hidden operands
 * (sh+ = sum P+), dW = V+^T H+ - V-^T H-, dv = (sv+ - sv-) / n, dh = (sh+ - sh-) / n:
 *   1. mode 0 (data):  mv = sv+ / n, mh = sh+ / n;     mode 1 (enhanced):  mv = (sv+ + sv-) / (2 n), mh = (sh+ + sh-) / (2 n)
 *   2. mu' = (1 - slide) mu + slide mv,   lam' = (1 - slide) lam + slide mh          (the model does not depend on the offsets:
 *      moving them transforms no parameter)
 *   3. gW = dW / n - mu' dh^T - dv lam'^T,   gb = dv - gW lam',   gc = dh - gW^T mu'
 *   4. W_m = mom W_m + lr (gW - wd W), W += W_m;   hb_m = mom hb_m + lr gc [- lr (sh+ / n - target) when o->sparsity],
 *      hid_bias += hb_m;   vb_m = mom vb_m + lr gb, vis_bias += vb_m
 *   5. mu := mu', lam := lam'
 * With mu = lam = 0 and slide = 0 this is the update of imdbn_rbm_cd_step / imdbn_rbm_pcd_step.
 * Launches, plain, on `stream`, no host sync: the phases, the statistics pass of the update kernel into `scratch`, centered_apply,
 * centered_finish.  No floating-point atomics; every sum has an order fixed by (V, H) and the grid, the grid depends on (V, H) and
 * the device's CU count only: the same call on the same state gives the same bits.  The row padding of W / W_m is neither read
 * nor written.  o->data_binary as in imdbn_rbm_cd_step; the prefetch fields and fwd_out must be zero.
 * scratch: device, imdbn_centered_scratch_floats(V, H) floats (the V H statistics, then the column and row partials of the bias
 * gradients), 16-byte aligned for the float4 kernels; contents unspecified on return.  Workspace: imdbn_ws_bytes(V, H, B).
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: a null momentum buffer, null data / o / mu / lam /
 * scratch, ldd < V, ldp < V with particles, B < 1, cd_k < 1 without particles or < 0 with them, a null rng where draws are needed,
 * slide outside [0, 1] or NaN, mode outside {0, 1}, a non-zero prefetch field or fwd_out; IMDBN_E_RNG: a replay tape shorter than
 * the draws. */
size_t imdbn_centered_scratch_floats(int V, int H);
int imdbn_rbm_centered_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, float* particles, int64_t ldp,
                            const imdbn_cd_opts* o, imdbn_rng* rng, float* mu, float* lam, float slide, int mode,
                            float* loss_out, float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- extended mean field: TAP training and log Z (imdbn/utils/tap.py; Gabrie, Tramel & Krzakala 2015) ------------
 * Bernoulli units on both sides, no softmax groups.  Magnetisations mv [B][V] (row stride ldmv >= V), mh [B][H] (ldmh >= H): device
 * fp32 in [0, 1], READ AND OVERWRITTEN in place; the padding of their rows is neither read nor written.  cv = mv - mv^2,
 * ch = mh - mh^2, W2 = fl32(W W) (made in registers, never stored); order 1 (naive mean field) drops every W2 term.
 *   hidden half-step    x = c + mv W - (mh - 1/2) o (cv W2),       mh <- damp mh + (1 - damp) sigmoid(x)
 *   visible half-step   y = a + mh W^T - (mv - 1/2) o (ch W2^T),   mv <- damp mv + (1 - damp) sigmoid(y)     (with the new mh)
 * One iteration = a hidden then a visible half-step.  The residual of a row: the largest |sigmoid(.) - m_old| over both half-steps
 * of the last iteration, before damping (0 with n_iters = 0).  Free energy of a row, with 0 ln 0 = 0:
 *   Gamma = sum_i [mv ln mv + (1 - mv) ln(1 - mv)] + sum_j [same for mh] - a.mv - c.mh - mv W mh^T - 1/2 cv W2 ch^T    (last: order 2)
 * and log Z ~ -Gamma at a fixed point.
 * imdbn_rbm_tap_iterate: n_iters >= 0 iterations, then out_gamma (double [B], nullable: one more weight pass) and out_res (float [B],
 *   nullable) of the state as it stands.  The caller's parameters are only read.
 * imdbn_rbm_tap_step: one update with n = B.  Positive phase as imdbn_rbm_cd_step (data V+, H+ = sigmoid(c + V+ W)); negative phase:
 *   n_iters >= 0 iterations on mv, mh;  gW = (V+^T H+ - mv^T mh - W o (cv^T ch)) / n  (last term: order 2, W before this update),
 *   ga = (sum V+ - sum mv) / n, gc = (sum H+ - sum mh) / n, then the momentum / weight-decay / sparsity rule of imdbn_rbm_cd_step.
 *   loss_out (nullable: that propagation is then not launched) = the mean-field reconstruction error of the data, as
 *   imdbn_rbm_pcd_step.  o->cd_k is not read; o->data_binary as in imdbn_rbm_cd_step; the prefetch fields and fwd_out must be zero.
 *   scratch: device, imdbn_rbm_tap_scratch_floats(V, H) floats (the statistics, then cv^T ch), 16-byte aligned for the float4
 *   kernels; contents unspecified on return.
 * Plain launches (and one memset node) on `stream`, no host sync, no allocation.  No floating-point atomics; every sum has an order
 * fixed by (V, H, B) and the device's CU count: the same call on the same state gives the same bits.  The row padding of W / W_m is
 * neither read nor written.  Workspace: 256-byte aligned, imdbn_rbm_tap_ws_bytes(V, H, B); nothing in it needs to survive a call.
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: a null d / parameter / (tap_step) momentum buffer,
 * softmax groups, null mv / mh / ws / (tap_step) data / o / scratch, a leading dimension below its row length, B < 1, n_iters < 0,
 * order outside {1, 2}, damp outside [0, 1) or NaN, a short or misaligned workspace, a short scratch, a non-zero prefetch field. */
size_t imdbn_rbm_tap_ws_bytes(int V, int H, int B);
size_t imdbn_rbm_tap_scratch_floats(int V, int H);
int imdbn_rbm_tap_iterate(const imdbn_rbm_desc* d, float* mv, int64_t ldmv, float* mh, int64_t ldmh, int B, int n_iters, float damp,
                          int order, double* out_gamma, float* out_res, void* ws, size_t ws_bytes, imdbn_stream_t stream);
int imdbn_rbm_tap_step(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, float* mv, int64_t ldmv, float* mh, int64_t ldmh,
                       const imdbn_cd_opts* o, int n_iters, float damp, int order, float* loss_out, float* scratch, size_t scratch_floats,
                       void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- deep Boltzmann machine: one half-step of a layer that hears from below and from above (imdbn/models/dbm.py; Salakhutdinov &
 *      Hinton 2009) ----------------------------------------------------------------------------------------------
 *   pre[b][n] = s_lo sum_k x_lo[b][k] W_lo[k][n] + s_hi sum_j x_hi[b][j] W_hi[n][j] + bias[n],   p = sigmoid(pre)
 * Raw device pointers, fp32: W_lo [K_lo][ldw_lo] (ldw_lo >= N: the lower RBM's W, the layer is its columns), W_hi [N][ldw_hi]
 * (ldw_hi >= K_hi: the upper RBM's W, or a row block of it; the layer is its rows), x_lo [B][K_lo] (ldx_lo >= K_lo), x_hi [B][K_hi]
 * (ldx_hi >= K_hi), bias [N].  A side is absent with x = NULL or K = 0 (its W and scale are then not read); both absent is an error.
 * mode: IMDBN_PARITY_F32 | IMDBN_FAST_BF16 as imdbn_rbm_desc.mode; both run the same fp32 arithmetic here.
 * Arithmetic: fp32 fused multiply-adds.  The reduction axis is [0, K_lo) ++ [0, K_hi), cut into slices of equal length (a multiple
 * of 32 steps; a function of K_lo + K_hi, N, B and the device's CU count).  Per slice the products of each side are added in index
 * order, the finished side sums are scaled (s_lo, s_hi meet sums, never products) and added, lo first; the slices are added in slice
 * order by the block that arrives last (an integer counter, left at zero); then the bias.  No floating-point atomics: the same call
 * gives the same bits.
 *   mean field (m != NULL, s == NULL): m [B][N] (ldm >= N) is READ AND OVERWRITTEN: m <- damp m + (1 - damp) p, damp in [0, 1).
 *     res (float [B], nullable): max_n |p - m_old| of every row, before damping.  rng is not read.
 *   sample (s != NULL, m == NULL): s [B][N] (lds >= N) = 1[p > U], U the call's one ("u", N) draw: PHILOX keyed on (seed, draw,
 *     row0 + b, n), REPLAY B N floats of the tape; rng->tape_used / draws_used (= 1) are filled in.  p (nullable, ldp >= N): the
 *     probabilities.
 * Row padding (of either W, of x, m, s, p) is neither read nor written.  Plain launches (and one memset node when the axis is split)
 * on `stream`, no host sync, no allocation.  Workspace: 256-byte aligned, imdbn_dbm_layer_ws_bytes(K_lo, K_hi, N, B) (0 for shapes
 * the call refuses); nothing in it needs to survive a call.
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: N < 1, B < 1, a negative K, both sides absent, a null
 * W of a present side, a null bias, a leading dimension below its row length, mode outside {0, 1}, both or neither of m / s, damp
 * outside [0, 1) or NaN, a null rng in sample mode, a misaligned workspace; IMDBN_E_WORKSPACE: a null or short workspace;
 * IMDBN_E_RNG: a replay tape shorter than the draw. */
size_t imdbn_dbm_layer_ws_bytes(int K_lo, int K_hi, int N, int B);
int imdbn_dbm_layer(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo, float s_lo,
                    const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi, float s_hi,
                    const float* bias, int N, int B, int mode,
                    float* m, int64_t ldm, float damp, float* res,
                    imdbn_rng* rng, float* s, int64_t lds, float* p, int64_t ldp,
                    void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- deep Boltzmann machine as a density model: annealed importance sampling over the odd layers and the layer term of the
 *      variational bound (imdbn/utils/likelihood.py: estimate_dbm_log_partition, dbm_variational_bound; Salakhutdinov & Hinton 2009,
 *      section 4.1) ---------------------------------------------------------------------------------------------
 * imdbn_dbm_rowsum_layer: the operands, the arithmetic and the summation order of pre are imdbn_dbm_layer's with s_lo = s_hi = 1.
 * Per batch row the call ADDS one double to acc[b] (float64 [B]), summed per tile of 64 units in a fixed butterfly and over the tiles
 * in tile order by one thread per row: no floating-point atomics, the same call gives the same bits.
 *   IMDBN_DBM_WEIGH   acc[b] += sum_n sp(e_n(beta)) - sp(e_n(beta_prev)),  e(t) = t pre + (1 - t) base_n in double from the fp32 pre
 *                     (base [N], nullable = zeros), sp(t) = max(t, 0) + log1p(exp(-|t|)); 0 <= beta_prev < beta <= 1.  With s != NULL
 *                     the units are also drawn at beta, as SAMPLE draws them (s NULL: the weight only, rng is not read).
 *   IMDBN_DBM_SAMPLE  p = sigmoid(fl(fl(beta pre) + fl(fl(1 - beta) base_n))) in fp32 (base NULL: fl(beta pre)), s [B][N] = 1[p > U],
 *                     U the call's one ("u", N) draw (PHILOX keyed on (seed, draw, row0 + b, n), or REPLAY B N floats); p nullable.
 *                     At beta = 1 without a base, s and p are imdbn_dbm_layer's sample mode bit for bit.  acc (nullable):
 *                     acc[b] += dbeta_next sum_n bias_n s_n.
 *   IMDBN_DBM_BOUND   one-sided from below (K_hi = 0): acc[b] += sum_n mu[b][n] pre[b][n] + h(mu[b][n]), h the Bernoulli entropy
 *                     (h(0) = h(1) = 0), mu [B][N] (ldmu >= N).  Here base (nullable) is the bias of the layer BELOW, [K_lo]:
 *                     acc[b] += sum_k base_k x_lo[b][k] first (one wave per row, lane l the terms l, l + 64, .. in order, butterfly).
 * Workspace: 256-byte aligned, imdbn_dbm_rowsum_layer_ws_bytes(K_lo, K_hi, N, B) (0 for shapes the call refuses).  Plain launches
 * (one memset node when the axis is split), no host sync, no allocation.  Padding is neither read nor written.
 * Errors as imdbn_dbm_layer, before the first launch, nothing touched; further IMDBN_E_INVALID: a mode outside the three, beta
 * outside [0, 1], beta_prev outside [0, beta), a null s in SAMPLE, p without s, s or p or a hi side in BOUND, a null mu or ldmu < N
 * in BOUND, a null acc in WEIGH / BOUND.
 *
 * imdbn_dbm_ais: M chains of a DBM of L + 1 layers (sizes [L + 1], W [L] device pointers with pitches ldw [L], W[l] being
 * [sizes[l]][ldw[l]] with ldw[l] >= sizes[l + 1]; biases [L + 1] device pointers; the four arrays live on the HOST) from the base model
 * (no weights, biases zero but layer 0's, which is base [sizes[0]], nullable = zeros) through betas [K + 1] (host; 0 = betas[0] < ..
 * < betas[K] = 1).  The state is the odd layers; the even ones are summed out.  Start: odd layers 1[0.5 > U], one ("u", N_l) each,
 * bottom first.  For k = 1 .. K: logw[m] += (beta_k - beta_{k-1}) sum_{l odd} b_l s_l + sum_{l even} WEIGH_l(beta_k, beta_{k-1}); for
 * k < K the transition at beta_k: every even layer bottom to top (drawn inside its WEIGH pass), then every odd layer bottom to top
 * from the new even states.  Draws: M sum_{l odd} N_l + (K - 1) M sum_l N_l floats (imdbn/engine/rng.py: sched_dbm_ais).
 * log Z ~= sum_{l >= 1} N_l log 2 + sum_i sp(base_i) + logmeanexp(logw).  logw: float64 [M], written.  out_s (nullable): a host array
 * of L + 1 device pointers read at the odd entries only; a non-null entry l receives the final state of layer l, [M][ld_out[l]].
 * One memset node and plain launches on `stream`, no host sync, no allocation; workspace imdbn_dbm_ais_ws_bytes(L, sizes, M).
 * The argument checks are those of imdbn_rbm_ais, in its words, and run before the first launch. */
#define IMDBN_DBM_WEIGH 0
#define IMDBN_DBM_SAMPLE 1
#define IMDBN_DBM_BOUND 2
#define IMDBN_DBM_MAX_LAYERS 16
size_t imdbn_dbm_rowsum_layer_ws_bytes(int K_lo, int K_hi, int N, int B);
int imdbn_dbm_rowsum_layer(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo,
                           const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi,
                           const float* bias, int N, int B, int mode, float beta, float beta_prev, double dbeta_next,
                           const float* base, const float* mu, int64_t ldmu,
                           imdbn_rng* rng, float* s, int64_t lds, float* p, int64_t ldp, double* acc,
                           void* ws, size_t ws_bytes, imdbn_stream_t stream);
size_t imdbn_dbm_ais_ws_bytes(int L, const int* sizes, int M);
int imdbn_dbm_ais(int L, const float* const* W, const int64_t* ldw, const int* sizes, const float* const* biases, const float* base,
                  const float* betas, int K, int M, imdbn_rng* rng, double* logw, float* const* out_s, const int64_t* ld_out,
                  void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- multimodal deep Boltzmann machine: one half-step of a layer of CATEGORICAL units (imdbn/models/mdbm.py; Srivastava &
 *      Salakhutdinov 2012) -------------------------------------------------------------------------------------
 * The operands, their pitches, the split of the reduction axis and the summation order of
 *   pre[b][n] = s_lo sum_k x_lo[b][k] W_lo[k][n] + s_hi sum_j x_hi[b][j] W_hi[n][j] + bias[n]
 * are imdbn_dbm_layer's, bit for bit (the label layer of the multimodal DBM passes the hi side only, W_hi being the rows
 * [Dz, Dz + K) of the joint RBM's W).  The N units are tiled exactly by n_groups consecutive softmax groups: group g is the columns
 * [group_end[g - 1], group_end[g]) with group_end[-1] = 0 and group_end[n_groups - 1] = N (group_end: a HOST array);
 * 1 <= n_groups <= IMDBN_MAX_GROUPS, widths 2 .. 256.  Per row and group, in fp32:
 *   mx = max_j pre_j,  e_j = expf(pre_j - mx),  p_j = e_j / sum,  where sum adds, per lane l of one wave, the columns l, l + 64,
 *   l + 128, l + 192 of the group in that order and then the 64 lane sums in the xor butterfly 32, 16, .. 1.
 *   mean field (m != NULL, s == NULL): m <- damp m + (1 - damp) p in place; res (float [B], nullable) = max_n |p - m_old| over the
 *     whole row.  rng is not read.
 *   sample (s != NULL, m == NULL): one ("c", width) draw per group, in group order, from the categorical source of rng: REPLAY
 *     reads n_groups B indices of cat_tape, [g][b]; PHILOX walks the inverse CDF over clamp(p_j, 1e-8, 1) in column order (fp32,
 *     left to right) against U total, U the uniform of (seed, draw + g, row0 + b, 0), as imdbn_rbm_sample_visible does.  s [B][N]
 *     is the one-hot rows; p (nullable) the probabilities.  rng->cat_used / draws_used (= n_groups) are filled in.
 * The logits stay in the workspace: [memset] one layer launch and one finish launch on `stream`, no host sync, no allocation, no
 * floating-point atomics (the same call gives the same bits).  Padding is neither read nor written.  Workspace: 256-byte aligned,
 * imdbn_dbm_group_layer_ws_bytes(K_lo, K_hi, N, B) (0 for shapes the call refuses); nothing in it needs to survive a call.
 * Errors as imdbn_dbm_layer, in its words, before the first launch, nothing touched; further IMDBN_E_INVALID: n_groups outside
 * 1 .. IMDBN_MAX_GROUPS or a null group_end, a width outside 2 .. 256, ends that do not tile [0, N). */
size_t imdbn_dbm_group_layer_ws_bytes(int K_lo, int K_hi, int N, int B);
int imdbn_dbm_group_layer(const float* W_lo, int64_t ldw_lo, int K_lo, const float* x_lo, int64_t ldx_lo, float s_lo,
                          const float* W_hi, int64_t ldw_hi, int K_hi, const float* x_hi, int64_t ldx_hi, float s_hi,
                          const float* bias, int N, int B, int mode, int n_groups, const int* group_end,
                          float* m, int64_t ldm, float damp, float* res,
                          imdbn_rng* rng, float* s, int64_t lds, float* p, int64_t ldp,
                          void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- Gaussian visible units with learned variances (imdbn/models/grbm.py: GaussianRBM; Cho, Ilin & Raiko 2011) ----
 * The parameters of the descriptor plus logvar [V] (device), sigma_i^2 = exp(logvar_i); with u = v exp(-logvar):
 *     p(h_j | v) = sigmoid(c_j + (u W)_j),   p(v_i | h) = N(b_i + (h W^T)_i, sigma_i^2),
 *     F(v) = sum_i (v_i - b_i)^2 / (2 sigma_i^2) - sum_j softplus(c_j + (u W)_j)
 * Softmax groups: IMDBN_E_UNSUPPORTED.  All calls are plain launches on the caller's stream: no host sync, no allocation, no
 * floating-point atomics, every sum in an order fixed by the shapes and the device's CU count (the same call on the same state gives
 * the same bits); the row padding of W / W_m is neither read nor written.  An argument error names the offending value and touches
 * nothing.  Workspace: imdbn_ws_bytes(V, H, B).
 *   gauss_prop_up      out_prob = sigmoid(((v exp(-logvar)) W + c) / T); out_sample (nullable) = 1[out_prob > U], draws ("u", H).
 *   gauss_prop_down    out_mean = b + h W^T, bit for bit the logits_only output of imdbn_rbm_prop_down at T = 1; out_sample (nullable)
 *                      = out_mean + exp(logvar / 2) n, draws ("n", V).
 *   gauss_sample_visible   out = mean + exp(logvar / 2) n for a caller's mean [B][V], draws ("n", V); no workspace.
 *   gauss_free_energy  out_F [B] = F(v).
 *   gauss_cd_step      one CD-k update, n = B:
 *       u0 = data exp(-z); P0 = sigmoid(u0 W + c); h = 1[P0 > U]                                                      ("u", H)
 *       cd_k >= 1 times:  m = b + h W^T;  v = m + exp(z / 2) n with sample_v, else v = m                              ("n", V)
 *                         u = v exp(-z); P = sigmoid(u W + c); on every step but the last h = 1[P > U]                ("u", H)
 *       draws_used = cd_k (1 + sample_v).  With u1 / P1 / v of the last step, S = u0^T P0 - u1^T P1 (the update kernel's exact
 *       products), q0_i = sum_b (data_bi - b_i)^2, q1_i = sum_b (v_bi - b_i)^2, r_i = sum_j W_ij S_ij (W, b as on entry):
 *           gW = S / n,  gb = colsum(u0 - u1) / n,  gc = colsum(P0 - P1) / n,  gz_i = exp(-z_i) (q0_i - q1_i) / (2 n) - r_i / n
 *           W_m = mom W_m + lr (gW - wd W), W += W_m;  vb_m = mom vb_m + lr gb, vis_bias += vb_m;
 *           hb_m = mom hb_m + lr gc - [sparsity] lr (colsum(P0) / n - target), hid_bias += hb_m;
 *           lr_z != 0:  logvar_m = mom logvar_m + lr_z gz, logvar = min(max(logvar + logvar_m, z_lo), z_hi)
 *           (lr_z == 0: logvar and logvar_m -- which may then be NULL -- are not touched)
 *       loss_out (nullable) = mean((data - m_last)^2).  Of o: cd_k, lr, momentum, weight_decay, sparsity, sparsity_target are read;
 *       the prefetch fields and fwd_out must be zero; the data are always read as real.
 *       scratch: device, imdbn_gauss_scratch_floats(V, H, B) floats (the V H statistics, the [B][V] mean and u, the partials), 16-byte
 *       aligned for the float4 kernel.
 * IMDBN_E_INVALID: a null argument, a leading dimension below its row length, B < 1, cd_k < 1, NaN lr_z, z_lo > z_hi or NaN,
 * sample_v outside {0, 1}, a null rng where draws are needed, a non-zero prefetch field or fwd_out; IMDBN_E_RNG: a replay tape
 * shorter than the draws. */
int imdbn_rbm_gauss_prop_up(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int B, float T, imdbn_rng* rng,
                            float* out_prob, int64_t ldo, float* out_sample, int64_t lds, void* ws, size_t ws_bytes, imdbn_stream_t stream);
int imdbn_rbm_gauss_prop_down(const imdbn_rbm_desc* d, const float* logvar, const float* h, int64_t ldh, int B, imdbn_rng* rng,
                              float* out_mean, int64_t ldo, float* out_sample, int64_t lds, void* ws, size_t ws_bytes,
                              imdbn_stream_t stream);
int imdbn_rbm_gauss_sample_visible(const imdbn_rbm_desc* d, const float* logvar, const float* mean, int64_t ldm, int B, imdbn_rng* rng,
                                   float* out, int64_t ldo, imdbn_stream_t stream);
int imdbn_rbm_gauss_free_energy(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int B, float* out_F,
                                void* ws, size_t ws_bytes, imdbn_stream_t stream);
size_t imdbn_gauss_scratch_floats(int V, int H, int B);
int imdbn_rbm_gauss_cd_step(const imdbn_rbm_desc* d, float* logvar, float* logvar_m, const float* data, int64_t ldd, int B,
                            const imdbn_cd_opts* o, float lr_z, float z_lo, float z_hi, int sample_v, imdbn_rng* rng, float* loss_out,
                            float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- annealed importance sampling over Gaussian visibles (imdbn/utils/likelihood.py: estimate_gaussian_log_partition; DESIGN
 * section 30) ---------------------------------------------------------------------------------------------------------------------
 * M chains from the base-rate model A -- W = 0, c = 0, the variances of the RBM, visible bias b_A -- to the Gaussian-visible RBM of
 * (d, logvar) through the temperatures betas[0..K] (0 = betas[0] < ... < betas[K] = 1).  With z = logvar, u = v exp(-z), x = c + u W,
 * q_X(v) = sum_i (v_i - b_X,i)^2 / (2 exp(z_i)) the intermediate distribution is
 *     p*_beta(v) = exp(-(1 - beta) q_A(v) - beta q_B(v)) prod_j (1 + exp(beta x_j))
 *   v_1 = b_A + exp(z / 2) n, logw = 0                                                                                      ("n", V)
 *   k = 1 .. K:  logw += (beta_k - beta_{k-1}) sum_i (b_i - b_A,i) exp(-z_i) (v_i - (b_i + b_A,i) / 2)
 *                        + sum_j [softplus(beta_k x_j) - softplus(beta_{k-1} x_j)]          (both sums in double, one expression)
 *                k < K:  h = 1[sigmoid(beta_k x) > U]                                                                      ("u", H)
 *                        v = ((1 - beta_k) b_A + beta_k (b + h W^T)) + exp(z / 2) n        (fp32, in this order)            ("n", V)
 *   draws_used = 2 K - 1; Philox is keyed on the global row, so chain i is the same chain whatever M.
 *   log Z ~= log Z_A + logmeanexp(logw),  log Z_A = H log 2 + (V / 2) log 2 pi + sum_i z_i / 2.
 * base_vis_bias (nullable) [V]: b_A.  NULL means b_A = b, the RBM's own visible bias -- NOT zeros as in imdbn_rbm_ais: a Gaussian
 * base model centred on 0 is a useless start for data far from 0, and with b_A = b the visible sum vanishes.
 * logw: device double [M], written.  out_v (nullable) [M][V], row stride ldo: the final states v_K.  The parameters are only read.
 * Plain launches on the caller's stream: no host sync, no allocation, no memcpy, no atomics; every row's sums have one order fixed
 * by (V, H), so the same call on the same state gives the same bits.  Workspace: imdbn_ws_bytes(V, H, M).
 * An argument error names the offending value, comes before the first launch and leaves logw untouched.  IMDBN_E_INVALID: M < 1,
 * K < 1, betas[0] != 0, betas[K] != 1, betas not strictly increasing, a null logvar / betas / rng / logw, ldo < V with out_v;
 * IMDBN_E_WORKSPACE: a short workspace; IMDBN_E_UNSUPPORTED: softmax groups; IMDBN_E_RNG: a replay tape shorter than the draws. */
int imdbn_rbm_gauss_ais(const imdbn_rbm_desc* d, const float* logvar, const float* betas, int K, int M, const float* base_vis_bias,
                        imdbn_rng* rng, double* logw, float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- reverse annealed importance sampling over Gaussian visibles (imdbn/utils/likelihood.py: gaussian_reverse_ais_log_likelihood;
 * DESIGN section 33) -------------------------------------------------------------------------------------------------------------
 * The forward chain of imdbn_rbm_gauss_ais read as a generative model p_ann over real rows (v_1 ~ N(b_A, exp(z)), v_{k+1} ~
 * T_k(. | v_k) for k = 1..K, one transition at beta_K = 1 included; the sample is v_{K+1}), run backwards from the rows v [R][V]
 * (real, row stride ldv; the caller replicates a test row once per chain).  In the notation of imdbn_rbm_gauss_ais, with
 * t_v(v) = sum_i (b_i - b_A,i) exp(-z_i) (v_i - (b_i + b_A,i) / 2) and T_k: h = 1[sigmoid(beta_k x(v)) > U], then
 * v' = ((1 - beta_k) b_A + beta_k (b + h W^T)) + exp(z / 2) n (fp32, in this order) -- a Gibbs step of the joint at beta_k, its own
 * reversal:
 *   logw = -q_B(v) + sum_j softplus(x_j(v))                                                                          (= -F(v))
 *   for k = K..1:  u_k ~ T_k(. | u_{k+1})                                              (u_{K+1} = v)          ("u", H), ("n", V)
 *                  logw -= (beta_k - beta_{k-1}) t_v(u_k) + sum_j [softplus(beta_k x_j(u_k)) - softplus(beta_{k-1} x_j(u_k))]
 *                                                                                      (both sums in double, one expression)
 * logw [R] (device, double) is OVERWRITTEN; exp(logw) / Z_A is an unbiased estimate of the density p_ann(v), log Z_A = H log 2 +
 * (V / 2) log 2 pi + sum_i z_i / 2 (NOT included).  base_vis_bias NULL means b_A = b, as in imdbn_rbm_gauss_ais.  out_v (nullable):
 * the final state u_1 [R][V], row stride ldo >= V.  A row holding a non-finite element gets logw = NaN, that row only (checked on
 * the device).
 * Draws: K times ("u", H), ("n", V): draws_used = 2 K.  Sums, logits and the Philox key as in imdbn_rbm_gauss_ais: row i is the
 * same chain whatever R, no atomics, and the same call on the same state gives the same bits.
 * Plain launches on the caller's stream: no host sync, no allocation, no memcpy.  Workspace: imdbn_ws_bytes(V, H, R).
 * An argument error names the offending value, comes before the first launch and leaves logw and out_v untouched.  IMDBN_E_INVALID:
 * R < 1, K < 1, betas[0] != 0, betas[K] != 1, betas not strictly increasing, a null logvar / v / betas / rng / logw, ldv < V, ldo < V
 * with out_v; IMDBN_E_UNSUPPORTED: softmax groups; IMDBN_E_WORKSPACE: a short workspace; IMDBN_E_RNG: a replay tape shorter than
 * K R (H + V) floats.  The caller's parameters, logvar and v are only read. */
int imdbn_rbm_gauss_reverse_ais(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int R, int K,
                                const float* betas, const float* base_vis_bias, imdbn_rng* rng, double* logw, float* out_v, int64_t ldo,
                                void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- the bottom bracket of the DBN lower bound under a Gaussian visible layer (imdbn/utils/likelihood.py:
 * gaussian_dbn_sample_values) ---------------------------------------------------------------------------------------
 * imdbn_rbm_bound_step for the Gaussian-visible RBM of (d, logvar).  For every row of v [M][V] (real, row stride ldv), with
 * z = logvar, u = v exp(-z), x = hid_bias + u W, sp = softplus in double:
 *   h = 1[sigmoid(x) > U]                         -> out_h [M][H] fp32 0/1, row stride ldh (the decision of imdbn_rbm_gauss_prop_up's
 *                                                    sample under the same draw)
 *   m = vis_bias + h W^T
 *   acc[row] += -sum_i ((v_i - m_i)^2 exp(-z_i) / 2 + z_i / 2) - (V / 2) log 2 pi + E       log N(v; m, exp(z)) plus E of
 *                                                    imdbn_rbm_bound_step (IMDBN_BOUND_ENTROPY / IMDBN_BOUND_LOGQ) on x
 *   acc[M] (device, double) is only ADDED to (the caller zeroes it): E first, then the row's Gaussian sum, then the constant, two
 *   launches of one stream.  Every element of the Gaussian sum is formed in double from the fp32 v_i, m_i, z_i.
 * Draws: ("u", H): draws_used = 1.  Every sum runs in an order fixed by (V, H), the logits and the mean are those of the
 * propagations, and Philox is keyed on the row: row i is the same whatever M; no floating-point atomics.
 * Plain launches on the caller's stream: no host sync, no allocation, no memcpy.  Workspace: imdbn_ws_bytes(V, H, M).
 * An argument error names the offending value, comes before the first launch and leaves acc and out_h untouched.  IMDBN_E_INVALID:
 * M < 1, unknown mode, null logvar / v / rng / acc / out_h, ldv < V, ldh < H; IMDBN_E_UNSUPPORTED: softmax groups; IMDBN_E_RNG: a
 * replay tape shorter than the draw; IMDBN_E_WORKSPACE: a short workspace.  The caller's parameters, logvar and v are only read. */
int imdbn_rbm_gauss_bound_step(const imdbn_rbm_desc* d, const float* logvar, const float* v, int64_t ldv, int M, int mode,
                               imdbn_rng* rng, double* acc, float* out_h, int64_t ldh, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- one delta-rule step of a directed layer (imdbn/models/idbn.py: updown_step; the up-down / contrastive wake-sleep algorithm of
 * Hinton, Osindero & Teh 2006) -------------------------------------------------------------------------------------
 * A directed sigmoid layer predicts `target` from `in` through the descriptor's weights: N_in = V, N_out = H for IMDBN_DELTA_UP
 * (recognition), N_in = H, N_out = V for IMDBN_DELTA_DOWN (generative).  in [B][N_in], target [B][N_out]: fp32, 0/1 or real in [0, 1],
 * row strides ldi >= N_in, ldt >= N_out.
 *   a = hid_bias + in W (UP) | vis_bias + in W^T (DOWN)       the logits of imdbn_rbm_prop_up / imdbn_rbm_prop_down at T = 1 with
 *                                                             logits_only, bit for bit
 *   p = sigmoid(a) (fp32),  r = target - p
 *   out_rowlp[b] = sum_j (target_j a_j - softplus(a_j))       double [B], nullable: log p(target | in) of the factorial Bernoulli layer
 *                                                             (a real target: minus the cross-entropy; target = p: minus the entropy)
 * With o != NULL the update, g in the [V][H] layout of W:  UP g = in^T r / B,  DOWN g = r^T in / B;
 *   W_m = momentum W_m + lr (g - weight_decay W), W += W_m;   m = momentum m + lr colsum(r) / B, bias += m
 * for the PREDICTING bias and its momentum only (hid_bias / hb_m for UP, vis_bias / vb_m for DOWN); the other bias and its momentum
 * buffer are not touched.  Of o only lr, momentum and weight_decay are read; cd_k, sparsity, the prefetch fields and fwd_out must be
 * zero.  out_rowlp is evaluated on the parameters on entry; o == NULL evaluates only and writes no parameter.
 * Launches, plain, on `stream`, no host sync: the operand preparation of `in`, the logits propagation, delta_rows (one pass over the
 * logits: the planes of target and of -p the weight pass reads, the column partials of r, the row partials of out_rowlp),
 * delta_finish (bias, out_rowlp), the update kernel of imdbn_rbm_cd_step with the pairs (in, target) and (in, p).
 * Sums: softplus and the row sum in double -- per 64-column tile lane l takes column l, the 64 lanes meet in a fixed butterfly, the
 * tiles are added in ascending order: fixed by N_out, a row gives the same bits alone and inside any batch.  colsum(r): fp32, 8 rows
 * per partial in row order, the partials in index order.  g: the update kernel's exact products, in^T target - in^T p in one fp32
 * accumulator (r itself is never rounded into an operand).  No draws, no floating-point atomics; the same call on the same state
 * gives the same bits.  The row padding of W / W_m is neither read nor written.
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: null d / in / target, dir outside {0, 1}, ldi < N_in,
 * ldt < N_out, B < 1, o == NULL together with out_rowlp == NULL (nothing to do), with o: a null momentum buffer, a non-zero cd_k /
 * sparsity / prefetch field / fwd_out.  IMDBN_E_UNSUPPORTED: DOWN on a descriptor with softmax groups.
 * Workspace: imdbn_ws_bytes(V, H, B). */
#define IMDBN_DELTA_UP   0   /* recognition: in [B][V] predicts target [B][H] through W and hid_bias   */
#define IMDBN_DELTA_DOWN 1   /* generative:  in [B][H] predicts target [B][V] through W^T and vis_bias */
int imdbn_rbm_delta_step(const imdbn_rbm_desc* d, int dir, const float* in, int64_t ldi, const float* target, int64_t ldt, int B,
                         const imdbn_cd_opts* o /* NULL: evaluate only */, double* out_rowlp /* [B], nullable */,
                         void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- one back-propagation step through a sigmoid layer (imdbn/models/idbn.py: autoencoder_step; the autoencoder fine-tuning of
 * Hinton & Salakhutdinov 2006) --------------------------------------------------------------------------------------
 * The layer of the descriptor is read in one or both directions.  The up pair is (x_v [B][V], e_h [B][H]): the layer maps x_v through
 * W to hidden pre-activations and e_h is the error there.  The down pair is (x_h [B][H], e_v [B][V]): the layer maps x_h through W^T to
 * visible pre-activations and e_v is the error there.  Each pair is given whole or not at all (both pointers NULL); fp32, row strides
 * ldxv / ldev >= V, ldeh / ldxh >= H.  An error is the ASCENT direction at a pre-activation (for a cross-entropy output layer:
 * target - p); an input x is the sigmoid output of the layer before it.
 *   err_v_out = (e_h W^T) * x_v * (1 - x_v)     [B][V], row stride ldov >= V, nullable, needs the up pair:   the error at the
 *                                               pre-activations that produced x_v
 *   err_h_out = (e_v W) * x_h * (1 - x_h)       [B][H], row stride ldoh >= H, nullable, needs the down pair: ... that produced x_h
 * Both from the parameters on entry: every launch that reads W for them precedes the update on the stream.  The product carries no
 * bias: it is the logits-only propagation of imdbn_rbm_prop_down / imdbn_rbm_prop_up on a zero bias, bit for bit -- a real, signed
 * operand through whatever kernel route that propagation takes -- and the epilogue q * (x * (1 - x)) runs in fp32.
 * With o != NULL the update, g in the [V][H] layout of W:  g = (x_v^T e_h + e_v^T x_h) / B, an absent pair contributing nothing;
 *   W_m = momentum W_m + lr (g - weight_decay W), W += W_m;
 *   with the up pair:    hb_m = momentum hb_m + lr colsum(e_h) / B, hid_bias += hb_m
 *   with the down pair:  vb_m = momentum vb_m + lr colsum(e_v) / B, vis_bias += vb_m
 * a bias without its pair is not touched, and neither is its momentum.  Both pairs at once are the exact gradient step of a layer
 * whose weights are used in both directions (the tied top RBM of an unrolled stack).  Of o only lr, momentum and weight_decay are
 * read; cd_k, sparsity, the prefetch fields and fwd_out must be zero.  o == NULL back-propagates only and writes no parameter.
 * Launches, plain, on `stream`, no host sync, no draws, no allocation: per error output the operand preparation of the error rows, a
 * memset node that clears the zero bias, the logits-only propagation and backprop_apply; with o, per pair the operand preparation
 * of the input rows (their planes) and backprop_rows (one pass over the error rows: their planes, the column partials, and with one
 * pair only the zero planes of the other slot), then backprop_finish (the biases) and the update kernel of imdbn_rbm_cd_step with
 * (vpos, hpos) = (x_v, e_h) and (vneg, hneg) = (e_v, x_h), the hidden planes of the second pair stored as they are to be added.
 * Sums: colsum: fp32, 8 rows per partial in row order, the partials in index order.  g: the update kernel's exact products, both
 * pairs in one fp32 accumulator.  No floating-point atomics; every order is fixed by (V, H, B): the same call on the same state gives
 * the same bits.  The row padding of W / W_m is neither read nor written.
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: a null descriptor, half a pair, no pair at all,
 * err_v_out without the up pair or err_h_out without the down pair, o == NULL with both outputs NULL (nothing to do), a leading
 * dimension below its width, B < 1, with o: a null momentum buffer, a non-zero cd_k / sparsity / prefetch field / fwd_out.
 * IMDBN_E_UNSUPPORTED: a descriptor with softmax groups.
 * Workspace: imdbn_ws_bytes(V, H, B).  The planes and column partials of both pairs fit the layout of a CD pass (two visible and two
 * hidden plane slots, four column-partial buffers): no scratch argument is needed. */
int imdbn_rbm_backprop_step(const imdbn_rbm_desc* d,
                            const float* x_v, int64_t ldxv, const float* e_h, int64_t ldeh,   /* up pair:   x_v [B][V], e_h [B][H]; both or neither */
                            const float* x_h, int64_t ldxh, const float* e_v, int64_t ldev,   /* down pair: x_h [B][H], e_v [B][V]; both or neither */
                            int B, const imdbn_cd_opts* o /* NULL: back-propagate only */,
                            float* err_v_out, int64_t ldov,   /* nullable, needs the up pair   */
                            float* err_h_out, int64_t ldoh,   /* nullable, needs the down pair */
                            void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- one back-propagation step through a Gaussian visible layer (imdbn/models/idbn.py: gaussian_autoencoder_step) --
 * The bottom layer of a stack with Gaussian visibles in the unrolled autoencoder, in its two roles.  d, logvar (z, sigma_i^2 =
 * exp(z_i)) as in the imdbn_rbm_gauss_* calls; v [B][V] the data (always needed); all gradients are ascent directions on minus
 *     J = (1/B) sum_b sum_i [ (v_bi - m_bi)^2 exp(-z_i) / 2 + z_i / 2 ]
 * and come from the parameters on entry.
 *   down pair x_h [B][H] (the layer is the decoder's output):  m = b + x_h W^T, bit for bit imdbn_rbm_gauss_prop_down;
 *       e_0 = (v - m) exp(-z);  gW = e_0^T x_h / B;  gb = colsum(e_0) / B;  gzeta_i = exp(-z_i) sum_b (v_bi - m_bi)^2 / (2 B) - 1/2
 *       err_h_out (nullable) = (e_0 W) x_h (1 - x_h), the e_v imdbn_rbm_backprop_step expects one layer up
 *       loss_out (nullable, two floats) = J and mean((v - m)^2)
 *   up pair e_h [B][H] (the layer is the encoder's input, e_h the error at its hidden pre-activations):  u = v exp(-z);
 *       gW = u^T e_h / B;  gc = colsum(e_h) / B;  gz_i = -(1/B) sum_j W_ij (u^T e_h)_ij
 *   both pairs (a single tied layer): one weight pass over u^T e_h + e_0^T x_h, and logvar moves by gzeta + gz.
 * o != NULL, the update (lr, momentum, weight_decay are read; cd_k, sparsity, the prefetch fields and fwd_out must be zero):
 *   W_m = momentum W_m + lr (gW - weight_decay W), W += W_m;  with the up pair hb_m = momentum hb_m + lr gc, hid_bias += hb_m;  with the
 *   down pair vb_m = momentum vb_m + lr gb, vis_bias += vb_m (a bias without its pair is not touched, nor its momentum);
 *   lr_z != 0:  logvar_m = momentum logvar_m + lr_z g, logvar = min(max(logvar + logvar_m, z_lo), z_hi)
 *   (lr_z == 0: logvar and logvar_m -- which may then be NULL -- are not touched).
 * o == NULL evaluates only (err_h_out, loss_out) and writes no parameter.
 * Launches, plain, on `stream`, no host sync, no draws, no allocation: with the down pair the two launches of
 * imdbn_rbm_gauss_prop_down; gauss_bp_rows (one pass over v and m: e_0 row-major and as planes, u, the column partials, the loss
 * partials, the zero planes of an absent pair's slot); for err_h_out the sequence of imdbn_rbm_backprop_step (operand preparation of
 * e_0, memset node, bias-free logits-only propagation, backprop_apply); with o the operand preparations, backprop_rows of e_h, then
 * with the up pair the update kernel in its statistics mode and gauss_apply (which returns r_i = sum_j W_ij S_ij; with both pairs
 * the share of the down pair, t_i = sum_b e_0,bi (m_bi - b_i), is taken out: gz_i = -(r_i - t_i) / B), with the down pair alone the
 * update kernel as imdbn_rbm_backprop_step runs it; gauss_bp_finish last (biases, logvar, the two loss figures).
 * Sums: column partials over 8 rows in row order, added in index order; r as in imdbn_rbm_gauss_cd_step; the loss in double over the
 * blocks' fp32 tree sums.  No floating-point atomics, every order fixed by (V, H, B) and the CU count; the row padding of W / W_m is
 * neither read nor written.
 * scratch: device, imdbn_gauss_backprop_scratch_floats(V, H, B) floats, 16-byte aligned for the float4 kernel.  Workspace:
 * imdbn_ws_bytes(V, H, B).
 * IMDBN_E_INVALID (naming the value) before the first launch, nothing touched: a null logvar / v / scratch, no pair, err_h_out or
 * loss_out without the down pair, o == NULL with nothing to output, a leading dimension below its width, B < 1, NaN lr_z, z_lo > z_hi
 * or NaN, lr_z != 0 with a null logvar_m, with o: a null momentum buffer, a non-zero cd_k / sparsity / prefetch field / fwd_out.
 * IMDBN_E_UNSUPPORTED: a descriptor with softmax groups. */
size_t imdbn_gauss_backprop_scratch_floats(int V, int H, int B);
int imdbn_rbm_gauss_backprop_step(const imdbn_rbm_desc* d, float* logvar, float* logvar_m, const float* v, int64_t ldv,
                                  const float* e_h, int64_t ldeh,   /* up pair, nullable:   e_h [B][H] */
                                  const float* x_h, int64_t ldxh,   /* down pair, nullable: x_h [B][H] */
                                  int B, const imdbn_cd_opts* o /* NULL: evaluate only */, float lr_z, float z_lo, float z_hi,
                                  float* err_h_out, int64_t ldoh,   /* nullable, needs the down pair */
                                  float* loss_out,                  /* nullable, needs the down pair: {J, mean((v - m)^2)} */
                                  float* scratch, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- parallel tempering over persistent chains (Desjardins et al. 2010; Cho, Raiko & Ilin 2010) -----------------
 * state [R M][V]: fp32, 0/1, one-hot inside softmax groups, row stride lds >= V, IN PLACE; replica r owns the rows [r M, (r + 1) M)
 * and samples p_beta(v) ~ exp(beta b.v + S(beta, v)), S(beta, v) = sum_j softplus(beta x_j(v)), x(v) = c + v W, at beta = betas[r].
 * betas: HOST array of R floats, 0 < betas[0] < ... < betas[R - 1] = 1.  swap_try / swap_acc: device int64 [max(R - 1, 1)], ADDED
 * to (the caller zeroes them): proposals and acceptances of the pair (r, r + 1) at index r.
 * Sweep s = 0 .. n_sweeps - 1:
 *   1. one Gibbs step per replica at T = 1 / betas[r]: h = 1[sigmoid(beta x(v)) > U], v = sample_visible(visible_probs(h, T)) -- the
 *      propagations of imdbn_rbm_gibbs_step(sample_h = 1, sample_v = 1) on the replica's rows.  The draw tensors span all R M rows:
 *      ("u", H), ("u", V), ("c", w_g) per group, and Philox is keyed on the row within them.
 *   2. only when R >= 2: for every pair (r, r + 1) with r = s (mod 2), r + 1 < R, and every chain m, with u / u' the states of
 *      chain m in the replicas r / r + 1:
 *        Delta = (beta_{r+1} - beta_r) (b.u - b.u') + S(beta_r, u') + S(beta_{r+1}, u) - S(beta_r, u) - S(beta_{r+1}, u')
 *        the two rows are swapped  iff  log(U) < Delta,     U: ("u", 1) over all R M rows, read at the LOWER replica's row
 *      -- the Metropolis ratio of the two tempered marginals; a one-hot group is part of the state and needs nothing extra.  The
 *      ("u", 1) tensor is consumed every sweep, also when no pair has the sweep's parity.  The logits are those of one logits-only
 *      up propagation over all rows; the softplus sums run in fp32 over chunks of 128 hidden units and in double across the
 *      chunks, b.u - b.u' in double, the comparison in double: every order is fixed by (V, H); the counters are integer atomics,
 *      there are no floating-point atomics.  A row outside every pair of the sweep is not touched by the exchange.
 * draws_used = n_sweeps (2 + G + [R >= 2]).  R = 1 is n_sweeps Gibbs steps at T = 1: the bits of imdbn_rbm_gibbs_step on the same draws.
 * IMDBN_E_INVALID (naming the value), nothing launched: null state / betas / rng / swap_try / swap_acc, lds < V, R < 1, M < 1,
 * n_sweeps < 0, betas[0] <= 0, betas[R - 1] != 1, betas not increasing; IMDBN_E_UNSUPPORTED: R > 64; a REPLAY tape with R >= 2 and
 * more than one softmax group; IMDBN_E_RNG: a replay tape shorter than the draws.
 * Workspace: imdbn_ws_bytes(V, H, R M), and no less than imdbn_ws_bytes(V, H, M) (the replicas' steps; checked).  Parameters are only read. */
int imdbn_rbm_pt_sweep(const imdbn_rbm_desc* d, float* state, int64_t lds, int R, int M, const float* betas, int n_sweeps, imdbn_rng* rng,
                       int64_t* swap_try, int64_t* swap_acc, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- exact log Z and exact marginals by enumeration (imdbn/utils/likelihood.py: exact_log_partition) ----------
 * One side of the RBM -- E, n <= 30 units, bias e -- is enumerated: state s has unit k of E on iff bit k of s is set; the other side
 * -- S, D units, bias f -- is summed out in closed form.  side: 0 the smaller side (ties: hidden), 1 hidden, 2 visible.
 *   E hidden, Bernoulli visibles, softmax groups allowed (x = b + W h):
 *       log Z = LSE_h [ c.h + sum_{i outside groups} softplus(x_i) + sum_g LSE_{k in g} x_k ]
 *   E hidden, Gaussian visibles (logvar = z given; a = W h):
 *       log Z = sum_i (log 2 pi + z_i) / 2 + LSE_h [ c.h + sum_i (b_i a_i + a_i^2 / 2) exp(-z_i) ]
 *   E visible, Bernoulli, no groups (x = c + v W):
 *       log Z = LSE_v [ b.v + sum_j softplus(x_j) ]
 * out: device double [2] = {log Z, the log of the largest state weight (the same constant included)}.
 * vis_mean [V] / hid_mean [H] (fp32, both or neither): the exact model marginals.  With w(s) = exp(t(s) - LSE_s t(s)), t the bracket
 * above: E gets sum_s w(s) s_k; S gets sum_s w(s) sigmoid(x_i), inside a softmax group sum_s w(s) softmax_g(x)_k, and for Gaussian
 * visibles E[v_i] = sum_s w(s) (b_i + a_i).
 * Launches: one prep launch (the n columns or rows of W of side E into a dense [n][D] block; row padding is never read); per 2^22
 * states one walk launch, the high bits in ascending order (n <= 22: one); one finishing launch; with marginals the walk launches once
 * more and a second finishing launch.
 * Sums: a pre-activation x_i(s) is reached from f_i by at most n + 26 fp32 additions (a fresh base every 32 states from the set bits
 * k >= 5 in ascending order, then a Gray-code walk of the 5 low bits); the terms of S add in fp32 inside a chunk of 128 columns
 * (two per lane) and in double across chunks and lanes (fixed butterfly); e.s and t(s) are doubles.  The LSE over states keeps
 * (max, scaled sum) pairs in double per lane, joined over the wave, the block's four waves in wave order, and one slot per block and
 * launch; the finishing launch folds the slots in a fixed order.  The marginals add w(s) times the fp32 term in double, per block,
 * and the finishing launch adds the blocks in index order.  No floating-point atomics: the same call on the same state gives the
 * same bits, whatever the scratch held.  Parameters are only read; no draws, no host sync, no allocation, no memcpy.
 * scratch: device, imdbn_exact_scratch_bytes(V, H, side) bytes (0 for an argument the call would refuse), 256-byte aligned.  It
 * always holds room for the marginal partials: min(2^min(n, 22) / 128, 512) (D + 32) doubles.
 * IMDBN_E_INVALID, naming the value, before the first launch and with nothing touched: a null d / out / scratch, side outside 0..2,
 * scratch too small or misaligned, exactly one of vis_mean / hid_mean, side = 2 with a non-null logvar.  IMDBN_E_UNSUPPORTED: more
 * than 30 units on the enumerated side; the visible side enumerated with softmax groups or (side = 0, V < H) Gaussian visibles;
 * Gaussian visibles with softmax groups.  With imdbn_profile_enable the whole call is bracketed by one event pair. */
size_t imdbn_exact_scratch_bytes(int V, int H, int side);
int imdbn_rbm_exact_logz(const imdbn_rbm_desc* d, const float* logvar /* NULL: Bernoulli visibles */,
                         int side /* 0: the smaller side (ties: hidden); 1: hidden; 2: visible */,
                         double* out /* device [2]: log Z, log of the largest state weight */,
                         float* vis_mean /* nullable, [V] */, float* hid_mean /* nullable, [H] */,
                         void* scratch, size_t scratch_bytes, imdbn_stream_t stream);

/* ---- data-parallel split of the same update ------------------------------ */
/* packed layout (floats): [dW V*H][dc H][db V][sum P+ H][sq-err sum 1][pad to 4] */
size_t imdbn_packed_delta_floats(int V, int H);
/* K3a: un-normalised local statistics of rbm.py:199-209 into `packed` (no parameter is touched) */
int imdbn_rbm_cd_stats(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B,
                       const imdbn_cd_opts* o, imdbn_rng* rng, float* packed,
                       void* ws, size_t ws_bytes, imdbn_stream_t stream);
/* K3b: rbm.py:212-226 from the (all-reduced) packed statistics with n = global batch */
int imdbn_rbm_apply_delta(const imdbn_rbm_desc* d, const float* packed, int global_B,
                          const imdbn_cd_opts* o, float* loss_out, imdbn_stream_t stream);

/* ---- data-parallel "factor exchange" (alternative to cd_stats / all-reduce / apply_delta) -----------------
 * The factors of <= 64 rows (visible / hidden operand planes, column sums, error partials: ~7 MB at 10000 x 1500)
 * are 8x smaller than the fp32 delta-W (60 MB).  Every rank: cd_factors (the CD pass; the factor block stays in its
 * workspace at imdbn_factor_block's offset), all-gather of the blocks, apply_factors (the update kernel runs once
 * per rank block; identical arithmetic on every rank, replicas stay bit-identical).
 * Needs <= 64 rows per rank, 16-B aligned weight rows, no softmax groups (IMDBN_E_UNSUPPORTED otherwise). */
int    imdbn_factor_block(int V, int H, int B, size_t* offset, size_t* bytes);
int    imdbn_rbm_cd_factors(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, const imdbn_cd_opts* opts,
                            imdbn_rng* rng, void* ws, size_t ws_bytes, imdbn_stream_t stream);
int    imdbn_rbm_apply_factors(const imdbn_rbm_desc* d, const void* gathered, int n_ranks, size_t rank_stride,
                               int rows_per_rank, int global_B, const imdbn_cd_opts* opts, float* loss_out,
                               imdbn_stream_t stream);

/* Wire form of the factor block: the negative visible sample (always 0/1) and, with binary_data != 0, the data plane
 * travel as 1 bit per element (7.0 -> 5.8 / 2.1 MB per rank at 10000 x 1500).  pack: one full block (as left by
 * imdbn_rbm_cd_factors) -> one compact block of imdbn_factor_compact_bytes(); all-gather the compact blocks;
 * unpack: n_ranks compact blocks -> n_ranks full blocks for imdbn_rbm_apply_factors.  A plane that is declared binary
 * and is not poisons the update with NaN (fails loudly).  All pointers / strides 16-B aligned; a compact buffer must be
 * zero-initialised once before its first use. */
int    imdbn_factor_compact_bytes(int V, int H, int B, int binary_data, size_t* bytes);
int    imdbn_rbm_pack_factors(int V, int H, int B, int binary_data, const void* block, void* compact, imdbn_stream_t stream);
int    imdbn_rbm_unpack_factors(int V, int H, int B, int binary_data, const void* compact, size_t compact_stride, int n_ranks,
                                void* gathered, size_t full_stride, int planes_only, imdbn_stream_t stream);
/* The two halves of a data-parallel step as ONE call each (a binder's step is: cd_factors_wire, all-gather of the wire blocks,
 * apply_wire).  cd_factors_wire = cd_factors + pack_factors, and it honours the next-batch prefetch fields of imdbn_cd_opts
 * (next_data / next_slot / data_slot / next_binary) exactly as imdbn_rbm_cd_step does.  apply_wire = unpack_factors(planes_only)
 * + apply_factors_wire; `planes`: scratch of n_ranks x planes_stride bytes, planes_stride >= imdbn_factor_block's size. */
int    imdbn_rbm_cd_factors_wire(const imdbn_rbm_desc* d, const float* data, int64_t ldd, int B, const imdbn_cd_opts* opts,
                                 imdbn_rng* rng, int binary_data, void* wire, void* ws, size_t ws_bytes, imdbn_stream_t stream);
int    imdbn_rbm_apply_wire(const imdbn_rbm_desc* d, const void* wire, size_t wire_stride, int n_ranks, int rows_per_rank,
                            int global_B, int binary_data, void* planes, size_t planes_stride, const imdbn_cd_opts* opts,
                            float* loss_out, imdbn_stream_t stream);
/* apply_factors reading the blocks' head (everything before the visible planes: verbatim in the wire form) straight
 * from the gathered wire blocks and the visible planes from the buffer unpack(planes_only = 1) expanded them into
 * (full-block layout, planes_stride apart): no copy of the 1.9 MB head per rank. */
int    imdbn_rbm_apply_factors_wire(const imdbn_rbm_desc* d, const void* wire, size_t wire_stride, const void* planes,
                                    size_t planes_stride, int n_ranks, int rows_per_rank, int global_B,
                                    const imdbn_cd_opts* o, float* loss_out, imdbn_stream_t stream);

/* ---- K4: conditional chains (rbm.py:240-400) -------------------------------------------- */
/* v0 = v_known*mask + (1-mask)*U (init_uniform=1) or v_known (0); then n_steps steps; out_v[B][V].
 * mu (nullable) is the [B][Dz] pull target of rbm.py:359-363. */
int imdbn_rbm_chain(const imdbn_rbm_desc* d, const float* v_known, const float* mask, int64_t ldk, int B,
                    int init_uniform, int n_steps, const imdbn_chain_step* steps,
                    const float* mu, int64_t ldmu, int Dz, imdbn_rng* rng,
                    float* out_v, int64_t ldo, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* Two independent chains of the same RBM and batch size as ONE call (iMDBN._cross_reconstruct, imdbn.py:419-449: its IMG->TXT
 * and TXT->IMG chains share nothing but the read-only weights).  Equivalent, bit for bit, to imdbn_rbm_chain(a) followed by
 * imdbn_rbm_chain(b) on the same rng; where the row-parallel chain kernel applies the two run in one launch, side by side. */
typedef struct imdbn_chain_spec {
    const float* v_known; const float* mask; int64_t ldk;   /* [B][V] clamp values and 0/1 mask (same row stride) */
    int32_t init_uniform; int32_t n_steps; const imdbn_chain_step* steps;
    const float* mu; int64_t ldmu; int32_t Dz; int32_t _pad; /* mu-pull target [B][Dz] (nullable) */
    float* out_v; int64_t ldo;                              /* final visible state [B][V] */
} imdbn_chain_spec;
int imdbn_rbm_chain_pair(const imdbn_rbm_desc* d, int B, const imdbn_chain_spec* a, const imdbn_chain_spec* b,
                         imdbn_rng* rng, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- convergence traces of conditional chains (imdbn/utils/conditional_steps.py) ------------------------------------
 * imdbn_rbm_chain_traced = imdbn_rbm_chain(a) (b == NULL) or imdbn_rbm_chain_pair(a, b), recording at every step the visible
 * probability p the step computes (after the mu-pull, BEFORE re-clamping and sampling) of the columns [c0, c1).  Recording only
 * observes: the final states, the draws and draws_used are those of the untraced calls, bit for bit.  A NULL trace records
 * nothing. */
typedef struct imdbn_chain_trace {
    int32_t c0, c1;          /* visible columns recorded, [c0, c1) */
    int32_t with_baseline;   /* 1: slot 0 = p(v | p(h | v0)) at T = 1 -- no sampling, no state change, no draws */
    int32_t _pad;
    float*  out;             /* slot s, row b at out + s*step_stride + b*ld_row; slots = n_steps + with_baseline */
    int64_t ld_row, step_stride;
} imdbn_chain_trace;
int imdbn_rbm_chain_traced(const imdbn_rbm_desc* d, int B, const imdbn_chain_spec* a, const imdbn_chain_trace* ta,
                           const imdbn_chain_spec* b, const imdbn_chain_trace* tb, imdbn_rng* rng,
                           void* ws, size_t ws_bytes, imdbn_stream_t stream);
/* imdbn_rbm_chain_traced (va / vb as ta / tb there) that can also record the HIDDEN probabilities (the joint-hidden trajectories of
 * imdbn/utils/bimodal_logging.py).  ha / hb (nullable) reuse imdbn_chain_trace over hidden columns [c0, c1) within [0, H): slot t
 * (0-based, n_steps slots) = sigmoid((v W + c + sigma * noise) / T) as step t computes it, with that step's T and noise -- the
 * probability BEFORE sampling, never the sample.  with_baseline must be 0 in a hidden trace (IMDBN_E_INVALID); a baseline in the
 * visible trace of the same chain shifts only the visible slots and writes nothing to the hidden trace.  Recording only observes,
 * as above; with ha == hb == NULL this IS imdbn_rbm_chain_traced. */
int imdbn_rbm_chain_traced_vh(const imdbn_rbm_desc* d, int B, const imdbn_chain_spec* a, const imdbn_chain_trace* va,
                              const imdbn_chain_trace* ha, const imdbn_chain_spec* b, const imdbn_chain_trace* vb,
                              const imdbn_chain_trace* hb, imdbn_rng* rng, void* ws, size_t ws_bytes, imdbn_stream_t stream);
/* IMG->TXT scan of a label trace of T steps after a baseline (slot 0), rows of K <= 256 probabilities (conditional_steps.py:40-130).
 * Per step, [B][T]: p_top1, p_top2, k1, k2 (ties to the lower index), p_gt (gt nullable; then p_gt may be NULL), l1 = |y_t - y_{t-1}|_1.
 * Per row: steps = first t with l1 < eps_l1, argmax streak >= stable_steps and p1 - p2 >= gap_thresh (T + 1: never); pred = argmax
 * at that step (at step T without convergence). */
int imdbn_trace_label_scan(const float* trace, int64_t step_stride, int64_t ld_row, int T, int B, int K, const int32_t* gt,
                           double eps_l1, int stable_steps, double gap_thresh, float* p_top1, float* p_top2, int32_t* k1,
                           int32_t* k2, float* p_gt, float* l1, int32_t* steps, int32_t* pred, imdbn_stream_t stream);
/* TXT->IMG code scan (conditional_steps.py:195-215): z_new[T][B][Dz] = (1-beta) z_prev + beta z_t (beta > 0) or z_t, starting from
 * z_init[B][Dz]; dz[B][T] = ||z_new_t - z_prev||_2. */
int imdbn_trace_code_scan(const float* trace, int64_t step_stride, int64_t ld_row, int T, int B, int Dz, const float* z_init,
                          int64_t ld_init, float ema_beta, float* z_new, float* dz, imdbn_stream_t stream);
/* TXT->IMG stop rule (conditional_steps.py:217-234) over dz[B][T] and mse[B][T]: steps[B] (T + 1: never) and best_mse[B]. */
int imdbn_trace_patience_scan(const float* dz, const float* mse, int T, int B, double eps_z, double mse_tol, int patience,
                              int32_t* steps, float* best_mse, imdbn_stream_t stream);
/* out_mse[i] = mean_c (p(v|h_i)_c - ref[ref_row[i]]_c)^2 with p(v|h) computed exactly as imdbn_rbm_prop_down at T = 1 (ref_row
 * nullable: row i).  The decoded rows stay in the workspace; the per-row sums run in a fixed order (deterministic).  No softmax groups. */
int imdbn_rbm_prop_down_sqerr(const imdbn_rbm_desc* d, const float* h, int64_t ldh, int B, const float* ref, int64_t ldr,
                              const int32_t* ref_row, float* out_mse, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- latent nearest-neighbour search (imdbn/utils/imdbn_logging.py) ---------------------------------------------------
 * imdbn_row_stats: out_sum[r] = sum_c x[r][c], out_sumsq[r] = sum_c x[r][c]^2 in fp32, in a fixed order (the same bits on every
 * call; exact integers for 0/1 rows).  Either output may be NULL, not both.
 *
 * imdbn_latent_topk: for every query row q, the first k candidates of the bank rows b in rank order.
 *   score   metric 0 (cosine): <q / max(|q|, 1e-12), b / max(|b|, 1e-12)>; 1 (inner): <q, b>;
 *           2 (l2): -((|q|^2 + |b|^2) - 2 <q, b>), the expansion (not clamped, not the direct difference).
 *           <q, b> is one k-ordered fp32 fma chain (zero-padded to a multiple of 32): a (query row, bank row) pair scores the
 *           same bits whatever Q, N, k or the other rows -- identical bank rows tie exactly.
 *   rank    score descending, the lower bank index on ties; NaN scores are never candidates.
 *   exclude [Q] nullable: bank row exclude[q] (-1: none) is not a candidate of query q.
 *   key     [N][2] nullable: only the best-ranked row of each exactly equal key pair is a candidate (the reference's
 *           dedup="image" walk over the sorted scores).
 *   out     out_idx[Q][k] (int32), out_score[Q][k]; fewer than k candidates: padded with -1 / -inf.
 *   bank_sumsq [N] nullable: |b|^2 as imdbn_row_stats gives it (metrics 0 / 2; computed into the workspace when NULL).
 *   Limits: 1 <= k <= 64 (IMDBN_E_INVALID otherwise), N, D, Q >= 1, ldb, ldq >= D.
 *   Workspace: at least A(4 Q) + A(4 N) + 2 A(4 Q k) bytes, A(x) = x rounded up to 256 (IMDBN_E_WORKSPACE below that);
 *           every further 2 A(4 Q k) bytes let the bank split into one more chunk (up to ceil(N / 64)) -- more blocks, the
 *           same result. */
int imdbn_row_stats(const float* x, int64_t ldx, int N, int D, float* out_sum, float* out_sumsq, imdbn_stream_t stream);
int imdbn_latent_topk(const float* bank, int64_t ldb, int N, int D, const float* bank_sumsq, const float* queries, int64_t ldq, int Q,
                      int metric, int k, const int32_t* exclude, const float* key, int32_t* out_idx, float* out_score, void* ws,
                      size_t ws_bytes, imdbn_stream_t stream);

/* ---- IMG->TXT energy trace (imdbn/utils/energy_utils.py; reference energy_utils.py:60-195) for a panel of N clamped codes ------
 * z[N][Dz] is the clamped code (columns [0, Dz) of the joint RBM `d`), the labels are columns [Dz, Dz + K), Wy = W[Dz:Dz+K].
 *   base  = z W[:Dz] + hid_bias: one K1 propagation (the logits path of imdbn_rbm_prop_up on the first Dz weight rows), then ONE kernel:
 *   F_k   = -(z.bz + by_k) - sum_j softplus(base_j + Wy[k][j]); kstar = argmin (lowest index on ties); margin_energy = F(2) - F(1);
 *           fe_top1 / fe_gap = top-1 and top-1 minus top-2 of softmax(-F).
 *   chain y_0 = y_start (NULL: uniform 1/K), pred_0 = argmax y_0, then for t = 1..steps
 *           h = sigmoid(base + y Wy), y_t = softmax(sigmoid(h Wy^T + by)) -- a softmax over the SIGMOID outputs of the label slice,
 *           whatever the descriptor's softmax groups say (the reference's step, energy_utils.py:69-79);
 *           per step [N][steps]: p_top1, p_top2, k1 (ties to the lower index), p_gt (gt nullable; then p_gt may be NULL),
 *           l1 = |y_t - y_{t-1}|_1, deltaF_pred = F[k1] - min F.
 *   stop    steps_to_converge = first t with l1 < eps_l1, argmax streak >= stable_steps and (k1 == kstar or p1 - p2 >= gap_thresh)
 *           (steps + 1: never); predT = k1 at that step (at the last step without convergence).  All `steps` run for every row.
 *   Every sum runs in a fixed order that depends on (Dz, K, H) only: a row gives the same bits alone or inside any panel.
 *   Limits: 2 <= K <= 256, Dz >= 1, Dz + K <= V, steps >= 1, ldz >= Dz, ldy >= K (IMDBN_E_INVALID otherwise).
 *   Workspace: imdbn_ws_bytes(Dz, H, N). */
typedef struct imdbn_energy_out {
    float*   p_top1; float* p_top2; float* p_gt; float* deltaF_pred; float* l1;   /* [N][steps] */
    int32_t* k1;                                                                   /* [N][steps] */
    int32_t* steps_to_converge; int32_t* kstar; int32_t* predT;                    /* [N] */
    float*   margin_energy; float* fe_top1; float* fe_gap;                         /* [N] */
    float*   F;                                                                    /* [N][K] */
    float*   y_final;                                                              /* [N][K], nullable: y after the last step */
} imdbn_energy_out;
int imdbn_energy_trace(const imdbn_rbm_desc* d, const float* z, int64_t ldz, int N, int Dz, int K, int steps, const int32_t* gt,
                       const float* y_start, int64_t ldy, double eps_l1, int stable_steps, double gap_thresh,
                       const imdbn_energy_out* out, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- cross-modal label metrics (imdbn/utils/cross_eval.py; reference imdbn.py:615-639, :764-813) for B rows of p(y | img) ----------
 * p[B][K] fp32 with row stride ldp >= K; only 4-byte alignment is assumed, so the tail view v[:, Dz:] of a chain result goes in as
 * it is.  The truth is exactly one of y[B][K] (ldy >= K; the first maximum of the row, as argmax) and gt[B] (int32).
 *   per row (each pointer nullable)
 *     pred    first maximum of p (the lower index on ties; NaN never wins);  gt = the truth as used;
 *     p_pred, p_true   p[pred], p[gt] clamped to [1e-9, 1];
 *     rank    #{j : p_j > p_gt} + #{j < gt : p_j == p_gt}: the place of the true label in a stable descending sort.
 *   accumulators -- ADDED to, never overwritten, so a loop over batches leaves one result (zero them before the first call)
 *     acc[8] (double, required): [0] rows, [1] top-1 hits (pred == gt), [2] top-k hits (rank < min(topk, K)),
 *             [3] ce_sum = -sum_rows [ log pt_gt + sum_{j != gt} log(1 - pt_j) ], pt = clamp(p, 1e-6, 1 - 1e-6) in fp32, logs in fp32
 *             (accurate logf), sums in double: F.binary_cross_entropy(reduction="sum") against the one-hot truth,
 *             [4] mse_sum = sum_rows row_mse * npix (row_mse[B] nullable: the output of imdbn_rbm_prop_down_sqerr),
 *             [5] skipped rows, [6], [7] untouched (zero);
 *     confusion[K][K] (int64, nullable): rows gt, columns pred;
 *     class_sums[K][3] (double, nullable): per true class rows, top-1 hits, sum of row_mse.
 *   A gt entry outside [0, K) is a caller error handled without a fault: the row enters no sum and no count but acc[5]; its
 *   p_true is NaN and its rank -1.
 *   Every floating-point sum runs in an order fixed by (B, K): the same batches leave the same bits (no floating-point atomics;
 *   the confusion counts are integer atomics).
 *   Limits: B >= 1, 2 <= K <= 256, topk >= 1, npix >= 1 (IMDBN_E_INVALID otherwise, naming the value).
 *   Workspace: 256-byte aligned, at least A(4 B) + 128 KiB bytes, A(x) = x rounded up to 256 (IMDBN_E_WORKSPACE below that). */
typedef struct imdbn_cross_metrics_out {
    int32_t* pred; int32_t* gt; float* p_pred; float* p_true; int32_t* rank;      /* [B] each, nullable */
    double*  acc;                                                                  /* [8] */
    int64_t* confusion;                                                            /* [K][K], nullable */
    double*  class_sums;                                                           /* [K][3], nullable */
} imdbn_cross_metrics_out;
int imdbn_cross_metrics(const float* p, int64_t ldp, int B, int K, const float* y, int64_t ldy, const int32_t* gt,
                        const float* row_mse, int npix, int topk, const imdbn_cross_metrics_out* out, void* ws, size_t ws_bytes,
                        imdbn_stream_t stream);

/* ---- pairwise free-energy scores of a joint RBM over [z1 (D1) | z2 (D2)], D2 = V - D1 (imdbn/utils/retrieval.py) ---------------
 * z1[Q][D1] (row stride ld1) are the queries, z2[N][D2] (ld2) the candidates; every (q, n) is scored in one sweep:
 *   S[q][n] = -F([z1_q | z2_n]) = z1_q . b[:D1] + z2_n . b[D1:] + sum_j softplus(c_j + (z1_q W[:D1])_j + (z2_n W[D1:])_j)
 *           a = c + z1 W[:D1] and b = z2 W[D1:] are the logits path of imdbn_rbm_prop_up on the two cuts of the descriptor; the two
 *           bias dots are fp32 sums in a fixed order; per pair the fp32 terms softplus(a_qj + b_nj) = max(x, 0) + log(1 + exp(-|x|))
 *           (hardware exp2 / log2) are added for j = 0 .. H - 1 in order into a double, and S is that total rounded to fp32.
 *           A (query row, candidate row) pair scores the same bits whatever Q, N, k, the workspace size, the outputs requested
 *           or the other rows; identical candidate rows tie exactly.  Error bound: DESIGN §28.
 *   rank_q[q] = #{n : S[q][n] > S[q][g]} + #{n < g : S[q][n] == S[q][g]}, g = gt_q[q]: the place of the true partner in a stable
 *           descending sort (the rule of imdbn_cross_metrics);  score_q[q] = S[q][g], the very bits the sweep gives that pair.
 *   rank_n[n], score_n[n]: the same over the column S[.][n] against S[gt_n[n]][n] -- the other direction from the same scores.
 *   top_idx[Q][k], top_score[Q][k]: per query the first k candidates in rank order (score descending, the lower index on ties,
 *           NaN never a candidate); fewer than k candidates: padded with -1 / -inf.
 *   scores[Q][N] (row stride lds), nullable: the whole matrix, for small panels and tests.  Without it no score reaches memory.
 *   A gt entry outside its range ([0, N) for gt_q, [0, Q) for gt_n) is a caller error handled without a fault: that row gets rank
 *   -1 and score NaN, nothing is read through it.  A NaN score is never greater than, equal to, or a candidate for anything.
 *   Integer counts, no floating-point atomics: the same call leaves the same bits.  No host synchronisation; parameters are read only.
 *   Limits (IMDBN_E_INVALID otherwise, naming the value, before the first launch and with no output touched): Q, N >= 1,
 *           1 <= D1 < V, ld1 >= D1, ld2 >= D2, lds >= N, 0 <= k <= 64, z1 / z2 / out not NULL, a rank or score output needs its gt,
 *           k > 0 needs top_idx and top_score, something must be requested.  Softmax groups: IMDBN_E_UNSUPPORTED.
 *   Workspace: 256-byte aligned, at least imdbn_pair_ws_bytes(V, H, Q, N, k) (IMDBN_E_WORKSPACE below that; 0 for arguments outside
 *           the limits).  Every further A(4 Q) + (k > 0 ? 2 A(4 Q k) : 0) bytes, A(x) = x rounded up to 256, let the candidates
 *           split into one more chunk (up to ceil(N / 64), about 2048 blocks in all) -- more blocks, the same result. */
typedef struct imdbn_pair_out {
    int32_t* rank_q;  float* score_q;          /* [Q], nullable; need gt_q */
    int32_t* rank_n;  float* score_n;          /* [N], nullable; need gt_n */
    int32_t* top_idx; float* top_score;        /* [Q][k], padded -1 / -inf; required iff k > 0 */
    float*   scores;  int64_t lds;             /* [Q][N] nullable, lds >= N: small panels and tests */
} imdbn_pair_out;
size_t imdbn_pair_ws_bytes(int V, int H, int Q, int N, int k);
int imdbn_rbm_pair_scores(const imdbn_rbm_desc* d, int D1, const float* z1, int64_t ld1, int Q,
                          const float* z2, int64_t ld2, int N, const int32_t* gt_q, const int32_t* gt_n, int k,
                          const imdbn_pair_out* out, void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- unit moments: sufficient statistics of act[B][H] for tuning curves and per-unit regressions (imdbn/utils/unit_tuning.py) ------
 * act[B][H] fp32 with row stride lda >= H (only 4-byte alignment is assumed; nothing beyond column H is read); cls[B] int32 is a
 * class per row (null with K = 0); x[B][R] fp32 with row stride ldx >= R are regressors (null with R = 0).  z = [1, x_1 .. x_R].
 *   A row is USED when its class lies in [0, K) (every row without cls) and its R regressors are finite.  Every other row is left
 *   out of every sum and counted in rows[1], so the curves and the regression describe the same rows.
 *   accumulators -- ADDED to, never overwritten, so a loop over batches leaves one result (zero them before the first call)
 *     cls_sum[K][H], cls_sumsq[K][H] (double), cls_count[K] (int64): per class sum a, sum a^2, rows (required with cls);
 *     xa[R + 1][H] (double): row q = sum z_q a over the used rows;   aa[H]: sum a^2;   xx[R + 1][R + 1]: sum z_p z_q;
 *     rows[2] (int64): used rows, skipped rows.  xa, aa, xx and rows are always required.
 *   Every product is formed in double from its fp32 factors (exact); every sum is a double sum in an order fixed by (B, H, K, R)
 *   and by which rows are used in which class (csrc/kernels_tuning.hpp): the same call leaves the same bits.  No floating-point
 *   atomics.  A non-finite activation poisons its own column only.  An accumulator row that receives no term (an empty class,
 *   a call whose rows are all skipped) is not written.  No host synchronisation.
 *   Limits (IMDBN_E_INVALID otherwise, naming the value, before the first launch and with no accumulator touched): B >= 1, H >= 1,
 *     0 <= R <= 8, 0 <= K <= 1024, K >= 1 with cls and K = 0 without, lda >= H, ldx >= R, x given exactly when R > 0, a null
 *     accumulator that the inputs require, ceil(H / 64) (max(K, 1) + ceil(B / 256)) + 81 above 2^31 - 1.
 *   Workspace: 256-byte aligned, at least imdbn_unit_moments_ws_bytes(B, H, K, R) (0 for arguments outside the limits); anything
 *     smaller is IMDBN_E_INVALID as well.  Its contents on entry do not matter. */
size_t imdbn_unit_moments_ws_bytes(int B, int H, int K, int R);
int imdbn_unit_moments(const float* act, int64_t lda, int B, int H, const int32_t* cls, int K, const float* x, int64_t ldx, int R,
                       double* cls_sum, double* cls_sumsq, long long* cls_count, double* xa, double* aa, double* xx, long long* rows,
                       void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- whole RBM.train_epoch_clamped (rbm.py:402-483) -------------------------------------- */
/* positive phase = chain(n_init steps) ; negative = cd_k steps from v+ ; update with o->lr */
int imdbn_rbm_clamped_step(const imdbn_rbm_desc* d, const float* v_known, const float* mask, int64_t ldk, int B,
                           int n_init, const imdbn_chain_step* init_steps,
                           const float* mu, int64_t ldmu, int Dz,
                           const imdbn_cd_opts* o, imdbn_rng* rng, float* loss_out,
                           void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* data-parallel half of the clamped update (reference statistics rbm.py:455-472): this rank's
 * un-normalised statistics in the packed layout of imdbn_rbm_cd_stats -> all-reduce (sum) ->
 * imdbn_rbm_apply_delta with o->sparsity = 0 (the clamped update has no sparsity term, rbm.py:473-481). */
int imdbn_rbm_clamped_stats(const imdbn_rbm_desc* d, const float* v_known, const float* mask, int64_t ldk, int B,
                            int n_init, const imdbn_chain_step* init_steps,
                            const float* mu, int64_t ldmu, int Dz,
                            const imdbn_cd_opts* o, imdbn_rng* rng, float* packed,
                            void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- K3 alone: the weight / bias update of rbm.py:209-224 from caller-supplied phase tensors ---------------------
 * W_m <- mom W_m + lr ((vpos^T hpos - vneg^T hneg)/B - wd W) ; W += W_m ; bias updates from the column sums (with the
 * sparsity term of rbm.py:217-219 when o->sparsity).  fp32 [B][V] / [B][H] inputs; no loss is computed. */
int imdbn_rbm_assoc_update(const imdbn_rbm_desc* d, const float* vpos, int64_t ldvp, const float* hpos, int64_t ldhp,
                           const float* vneg, int64_t ldvn, const float* hneg, int64_t ldhn, int B, const imdbn_cd_opts* o,
                           void* ws, size_t ws_bytes, imdbn_stream_t stream);

/* ---- C1: the data-parallel exchange over RCCL (xGMI) for binders that do not use torch.distributed ---------------
 * (the Python classes exchange through torch.distributed, whose "nccl" backend is the same RCCL).  One communicator
 * per process and GPU: rank 0 calls imdbn_comm_unique_id (128 bytes), the caller carries the id to every rank, every
 * rank calls imdbn_comm_init; then per CD step either imdbn_allreduce_sum_f32 on the packed statistics of
 * imdbn_rbm_cd_stats, or imdbn_allgather_bytes on the factor blocks.  librccl is opened on first use. */
int imdbn_comm_unique_id(void* id128);
int imdbn_comm_init(void** comm, int world, int rank, const void* id128);
int imdbn_comm_destroy(void* comm);
int imdbn_allreduce_sum_f32(void* comm, float* buf, size_t count, imdbn_stream_t stream);
int imdbn_allgather_bytes(void* comm, const void* send, void* recv, size_t bytes_per_rank, imdbn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IMDBN_ENGINE_H */
