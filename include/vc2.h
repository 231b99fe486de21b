/* vc2.h -- C ABI of the MI355X-native VidCom2 token-compression hot path (libvc2hip.so).
 *
 * The reference (xuyang-liu16/VidCom2) has no FFI: its boundary is the Python module
 * token_compressor/vidcom2/vidcom2.py.  Each entry point below names the reference function
 * (file:line) whose tensor work it replaces; vidcom2_amd/vidcom2.py binds them with ctypes
 * and re-exposes the reference's Python names and signatures.
 *
 * Conventions
 *   - plain pointers + sizes only; no torch / C++ types cross this boundary
 *   - every pointer is a DEVICE pointer unless the name says host; `stream` is a hipStream_t
 *     passed as void* (NULL = the legacy default stream)
 *   - functions only ENQUEUE work on `stream`; none of them synchronises, allocates or frees
 *     device memory (the caller passes a workspace sized by vc2_workspace_bytes)
 *   - return 0 on success, a negative VC2_ERR_* otherwise (nothing was enqueued on error);
 *     vc2_last_error() gives a thread-local message
 *   - dtype codes: 0 = fp32, 1 = bf16, 2 = fp16.  All arithmetic follows the reference's
 *     "every op in the input dtype" behaviour: each torch op is evaluated exactly and rounded
 *     fp32 -> T (DESIGN.md "Numerics contract"); index outputs are int64 like torch's
 *   - row-major contiguous tensors; 16-byte aligned base pointers
 *   - size limit: a row of D channels is read as D / 8 (16-bit) or D / 4 (fp32) 16-byte vectors, or as D
 *     scalars when D is not a multiple of that; at most 1024 of them.  So D <= 8192 for 16-bit and <= 4096 for
 *     fp32 when the row is whole vectors, D <= 1024 otherwise; a wider row gives VC2_ERR_UNSUPPORTED
 *     (vc2_workspace_bytes already refuses it)
 */
#ifndef VC2_H_
#define VC2_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC2_F32 0
#define VC2_BF16 1
#define VC2_F16 2

#define VC2_OK 0
#define VC2_ERR_ARG (-1)          /* bad argument (null pointer, non-positive size, bad dtype) */
#define VC2_ERR_SHAPE (-2)        /* rows not divisible by tokens-per-frame (torch .view RuntimeError) */
#define VC2_ERR_UNSUPPORTED (-3)  /* shape outside what the kernels cover (size limit above) */
#define VC2_ERR_LAUNCH (-4)       /* hipLaunch failure; message in vc2_last_error() */
#define VC2_ERR_WORKSPACE (-5)    /* workspace too small */

#define VC2_MAP_LINEAR 0          /* vidcom2.py:99-103  _map_linear_offset */
#define VC2_MAP_GRID_VID 1        /* vidcom2.py:105-115 _map_grid_vid      */
#define VC2_MAP_LOCAL 2           /* per-frame local indices (select_outlier_indices output) */

const char* vc2_last_error(void);
const char* vc2_version(void);

/* Accumulation semantics of the reference's fp32-accumulated reductions in half precision (token L2 norm,
 * squared-distance row sums, centre means):
 *   4 (default)  "torch order": wherever the exactly computed value lies within a margin of fp32-ulps of a T rounding
 *                boundary, torch's own CPU accumulation order (bf16: 8 interleaved fp32 chains over the variance-sorted
 *                channels, fp16: one sequential chain / cascade sum) is replayed for that token -> bit-exact to the CPU
 *                reference.  The margins (vc2_selftest_margins): squared-distance sums 48, a bound on the cascade's error;
 *                norms max(128, bound of torch's chains) for bf16, 128 for fp16 -- a bound up to 254 scored channels and an
 *                EMPIRICAL margin beyond: an fp16 row on which every add of torch's chain errs the same way (built inputs
 *                only; ordinary data errs by ~10 ulps) keeps the exactly rounded norm in this mode.  Mode 3 has the bound.  FRAME-centre means
 *                (round 6): the model shapes -- 16-bit inputs, D = 1024 / 3584 / 4096, frames of <= 512 tokens, every frame
 *                workgroup resident -- add every frame's x^ in torch's OWN order inside sweep 2 (16-row blocks, fp32, the
 *                outer-sum cascade of SumKernel.cpp): the frame means are the reference's bits by construction, no margin,
 *                no replay (environment VC2_S2_ORD=0: the form below).  Other shapes, and the VIDEO-centre mean everywhere:
 *                exact (fp64) sums, and a mean within 16 fp32-ulps of a T boundary is replayed in torch's order; for frame
 *                means the margin has, besides the 16 ulps, a term relative to sum |x^| over the frame (4 u A / n, A bounded
 *                from sweep 1's statistics and the frame's smallest denominator): it grows under cancellation, where torch's
 *                cascade errs by far more than ulps OF THE MEAN.  Reproduces the reference on every fixture (incl. the
 *                adversarial `cancel` ones) and every soak case.
 *   0            "exact": every reduction correctly rounded (DESIGN.md "Numerics contract").
 *   3            "proven": a PROVEN bound decides which centre means are replayed (forward error bound of torch's
 *                cascade relative to sum |x^|, bounded from sweep 1's statistics) and which fp16 norms (C / 2 + 1 ulps for C
 *                scored channels: a fifth of the rows at C = 1792): flags 50x more means, costs ~45 %
 *                more time (256 against 178 us per pass at the target shape, round 5; with VC2_S2_ORD=0); the test-suite runs every fixture
 *                in it as well and asserts the same results.
 *   1            "fast" (the default of rounds 1-3, now opt-in): the 16-ulp margin alone for all centre means.  ~1 %
 *                faster than mode 4 (176 against 178 us, round 5); NOT bit-exact under cancellation (0.2 % of random `cancel` inputs differ in last-bit
 *                f scores, rarely a kept index) -- no claim of reference parity is made for it.
 *   (2: debug -- every value is replayed.)
 * fp32 inputs are unaffected.  vc2_set_mode is PROCESS-WIDE (default 4) and also drops the calling thread's own
 * override; vc2_set_thread_mode(mode) overrides it for the calling thread only (-1: follow the process-wide setting
 * again), so that a worker thread follows the application's choice unless it asks otherwise; vc2_get_mode returns
 * what a pass issued by the calling thread would use.  (All ranks / threads of a frame-sharded pass must use the
 * same mode: it decides which exchanges take place.) */
int vc2_set_mode(int mode);
int vc2_set_thread_mode(int mode);
int vc2_get_mode(void);
/* Workspace (bytes) needed by any entry point below for an [F*N, D] input.
 *   - ONE size per (F, N, D, dtype): the numerics mode (process-wide or a thread's override) does not change it, so a
 *     workspace sized in one mode serves a pass issued in any other.  That one size also serves every variant of the pass:
 *     any vc2_pass_params, either score_dtype, every flag, both mappings and the frame-sharded options need the same
 *     layout or a smaller one (the whole video's frame count only lowers the number of sweep-1 row groups; fp32 scoring
 *     drops the replay engine's arrays).
 *   - Its CONTENTS ON ENTRY ARE IGNORED: uninitialised memory, another shape's leftovers, any bytes.  Every counter, status
 *     word, queue, mark, sentinel and list the kernels keep there is re-armed by the call itself before its first reader
 *     (DESIGN.md "Workspace regions: who writes before whom").  The one exception is what a call is TOLD to find there:
 *     sweep 1's partials under VC2_FLAG_HAVE_STATS (left by vc2_pool_stats), and, between the calls of ONE frame-sharded
 *     pass on one workspace, what its earlier calls left (vc2_chan_stats -> vc2_scores_phase1 -> vc2_video_centre_* ->
 *     vc2_scores_phase2* -> vc2_select_sharded).
 *   - A call writes only inside [ws, ws + vc2_workspace_bytes) and inside the stated extents of its outputs; with ws_bytes
 *     below the size it returns VC2_ERR_WORKSPACE and enqueues nothing.
 *   - The workspace belongs to the pass until the pass has finished on its stream: two passes in flight need two. */
int vc2_workspace_bytes(int64_t F, int64_t N, int64_t D, int dtype, size_t* out_bytes);

/* Upper bound on the number of kept tokens sum(ks) for a given base_scale: lets the caller
 * allocate the output of vc2_compress before the budgets are known (the reference learns K
 * from a host sync, vidcom2.py:72). */
int64_t vc2_kept_capacity(int64_t F, int64_t N, double base_scale);

/* ---- stage entry points ------------------------------------------------------------ */

/* vidcom2.py:40  x.var(dim=0, unbiased=False) -> var T[D] (also fp32-widened copy var_f32[D],
 * may be NULL).  Sweep 1 of X. */
int vc2_chan_var(const void* x, int64_t R, int64_t D, int dtype, void* ws, size_t ws_bytes,
                 void* var_T, float* var_f32, void* stream);

/* vidcom2.py:41-42  torch.topk(var, k, largest=False): the SET of the k selected channels, with ties
 * at the k-th value broken exactly like the CPU reference (libstdc++ introselect; SURVEY.md
 * Appendix A).  var_f32 = widened T values.  Outputs (each may be NULL): byte mask mask[D]
 * (1 = selected); the ascending channel list cols[k] the scoring sweeps consume; perm[k] = the selected channels
 * in the order nth_element / partial_sort left them (the input of the ORDER replay below).
 * With order / opos / spos (need perm; opos / spos also need cols) a second kernel replays torch.topk(sorted=True)'s
 * OWN order: order[k] = ascending variance, libstdc++ sort tie order -- the column order of `x[:, topk_idx]`,
 * vidcom2.py:43; opos[k] = position of order[p] inside cols; spos[k] = its inverse (position of cols[i] in that
 * order: what the "torch order" replays of the scoring sweeps need).  The fused pass and vc2_scores_phase1 do not
 * call this second kernel: they attach the same job to sweep 2 as a rider workgroup. */
int vc2_chan_select(const float* var_f32, int64_t D, int64_t k, uint8_t* mask, int32_t* cols, int32_t* perm,
                    int32_t* order, int32_t* opos, int32_t* spos, void* stream);

/* vidcom2.py:43  x[:, idx] column gather -> out T[R, C]; idx int64[C] on device. */
int vc2_gather_cols(const void* x, int64_t R, int64_t D, int dtype, const int64_t* idx, int64_t C,
                    void* out, void* stream);

/* vidcom2.py:45-62  compute_gaussian_scores over the C channels listed (ascending) in cols[C]
 * (cols NULL = all channels, C == D, i.e. x already holds the selected features, already in torch.topk
 * order).  spos = vc2_chan_select's output (needed for mode 1 when cols != NULL).  Sweeps 2 and 3 of X.
 * Outputs: v_T, f_T  T[F,N] (may be NULL), total_f32 fp32-widened RN_T(v+f) [F,N] (vidcom2.py:33),
 * s_f32[F] = -mean(v, -1) widened (vidcom2.py:32).
 * Cost note: in modes 3 and 4 (4 is the default) the frame-mean replay margins are bounded from the channel statistics
 * of x, so this stage call runs the statistics sweep (sweep 1) over x itself before sweeps 2 and 3 -- three sweeps, where
 * modes 0 / 1 take two.  The one-launch pass (vc2_compress*) and vc2_scores_phase1 behind vc2_chan_stats reuse sweep 1's
 * partials instead. */
int vc2_scores(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
               int64_t C, const int32_t* spos, void* ws, size_t ws_bytes, void* v_T, void* f_T,
               float* total_f32, float* s_f32, void* stream);

/* vidcom2.py:64-68  compute_scales(scores, base, temp) on T[F] -> scales T[F]. */
int vc2_compute_scales(const void* s_T, int64_t F, double base, double temp, int dtype, void* ws,
                       size_t ws_bytes, void* scales_T, void* stream);

/* vidcom2.py:72-77  ks = (scales*tpf).round().long().clamp(min=1); per frame the k_f smallest
 * total scores (CPU-reference tie-breaking), ascending.  map_mode selects the index mapping
 * fused into the output (VC2_MAP_*; grid_h only for GRID_VID).  Outputs: ks int64[F],
 * (tpf = the reference's multiplier, normally N; a k_f > N is reported raw in ks while min(k_f, N) tokens are
 * selected -- the caller raises torch.topk's "k out of range" error),
 * offs int64[F+1] (exclusive prefix of min(ks, N)), idx_out int64[cap] and K_out[0] = number of indices
 * written.  K_out[1] = status bits, all zero on a sound pass: 1 = the count would have exceeded `cap` (nothing past
 * cap is written), 2 = a bounded wait between workgroups of one launch of this pass expired, 4 = a loop bound of the
 * selection replay expired IN THIS PASS (any of its kernels: channel selection, ORDER riders, per-frame selection; the
 * one-launch pass keeps the bit in its own workspace word, so two passes in flight on two streams cannot report each
 * other's hits; vc2_selftest_counters has the process-wide details); the Python mirror raises on any of them.  Stage
 * calls (this function) report their own launch only: K_out[1] is zeroed before the launch and every workgroup that
 * sees a hit ORs it in (a hit of ANY frame's selection is reported, whichever workgroup wrote the count). */
int vc2_select(const void* scores_T, const void* scales_T, int64_t F, int64_t N, int64_t tpf, int dtype,
               int map_mode, int64_t grid_h, void* ws, size_t ws_bytes, int64_t* ks, int64_t* offs,
               int64_t* idx_out, int64_t cap, int64_t* K_out, void* stream);

/* vidcom2.py:99-103 / :105-115 as standalone mappers: local per-frame indices (concatenated,
 * with ks/offs) -> global indices. */
int vc2_map_indices(const int64_t* local_idx, const int64_t* ks, const int64_t* offs, int64_t F,
                    int map_mode, int64_t stride_or_h, int64_t* out, void* stream);

/* vidcom2.py:91 / :96  flat[global_idx]: dst[j,:] = src[idx[j],:] for j < K_dev[0] (K read on
 * device; at most `cap` rows). */
int vc2_gather_rows(const void* src, int64_t src_rows, int64_t D, int dtype, const int64_t* idx,
                    const int64_t* K_dev, int64_t cap, void* dst, void* stream);

/* vidcom2.py:93-96, :105-115  img_feat[_map_grid_vid(...)] without img_feat: idx[] holds indices into the
 * [F*h*(h+1), D] stream LLaVA-Video's add_token_per_grid builds (every grid row of every frame followed by the
 * image_newline embedding); out[j,:] = src[f*h*h + r*h + c,:] for g = idx[j] = f*h*(h+1) + r*(h+1) + c with c < h, and
 * the [D] vector `newline` for c == h; j < min(n_dev[0], n_max) (n_dev NULL: n_max).  src = the scored tensor
 * T[F*h*h, D]; the stream is never built.  An index outside [0, F*h*(h+1)) is skipped.  A null newline: VC2_ERR_ARG. */
int vc2_gather_rows_grid(const void* src, int64_t F, int64_t h, int64_t D, int dtype, const int64_t* idx,
                         const int64_t* n_dev, int64_t n_max, const void* newline, void* out, void* stream);

/* vidcom2.py:89-91  flat[global_idx] for a video that lies in n_chunks allocations (a vision tower that encodes a few
 * dozen frames at a time): idx[] holds rows of the virtual concatenation of the chunks, chunk c holding chunk_rows[c]
 * rows of D elements, and dst[j,:] = chunk_c[idx[j] - start_c,:] for j < min(n_dev[0], n_max) (n_dev NULL: n_max), c the
 * chunk with start_c <= idx[j] < start_c + chunk_rows[c], start_c = chunk_rows[0] + ... + chunk_rows[c-1].  chunks and
 * chunk_rows are HOST arrays (chunks[c]: a device pointer); the table reaches the kernel by value: no copy, no
 * synchronisation.  An index outside [0, sum chunk_rows) or a destination row j >= dst_rows is skipped and reported:
 * *status |= 2 (status: a device word the caller zeroed, or NULL).  Rows of any alignment (16 bytes per lane when the row
 * bytes and both addresses allow it).  n_chunks outside 1..VC2_RAGGED_MAX_WORLD: VC2_ERR_UNSUPPORTED; a null chunks /
 * chunk_rows / idx / dst or chunk pointer, or a chunk_rows entry < 1: VC2_ERR_ARG; nothing is enqueued. */
int vc2_gather_rows_chunks(const void* const* chunks /* host [n_chunks] device pointers */,
                           const int64_t* chunk_rows /* host [n_chunks] */, int n_chunks, int64_t D, int dtype,
                           const int64_t* idx, const int64_t* n_dev, int64_t n_max, void* dst, int64_t dst_rows,
                           int32_t* status, void* stream);

/* vidcom2.py:89-91, :93-96, :105-115 (the reference's models/llava.py:118-127)  vc2_gather_rows_chunks with the options
 * of the one-shot pass's gather.  h == 0: idx[] holds rows of the virtual concatenation, as there.  h > 0: idx[] holds
 * slots g = f*h*(h+1) + r*(h+1) + c of the [F_total*h*(h+1), D] stream add_token_per_grid would build over the virtual
 * concatenation (F_total = sum chunk_rows / (h*h)); dst[j,:] is the [D] vector `newline` for c == h and row
 * f*h*h + r*h + c of the concatenation otherwise -- neither the concatenation nor the stream is built.  In both spaces
 * `tail_rows` rows of `tail` are written behind row n = min(n_dev[0], n_max) (n_dev NULL: n_max).  An index outside its
 * space, or a destination row >= dst_rows, is skipped -- never read or written -- and reported: *status |= 2.  Chunk
 * bases, newline and tail of any alignment.  Codes as vc2_gather_rows_chunks, and VC2_ERR_ARG for h < 0, h > 0 with a
 * null newline or with a chunk_rows entry that is not a multiple of h*h, tail_rows < 0, tail_rows > 0 with a null tail;
 * nothing is enqueued. */
int vc2_gather_rows_grid_chunks(const void* const* chunks /* host [n_chunks] device pointers */,
                                const int64_t* chunk_rows /* host [n_chunks] */, int n_chunks, int64_t h, int64_t D,
                                int dtype, const int64_t* idx, const int64_t* n_dev, int64_t n_max, const void* newline,
                                const void* tail, int64_t tail_rows, void* dst, int64_t dst_rows, int32_t* status,
                                void* stream);

/* ---- one-shot hot path -------------------------------------------------------------- */

/* vidcom2.py:15-36  vidcom2_compression for the "linear" mapper (llava_ov / qwen*), and for
 * "grid_vid" when gather_src/map_mode say so: everything from the feature tensor resident in HBM
 * to kept rows + indices + budgets, enqueued back-to-back with no host round trip.
 *   x           T[F*N, D]
 *   gather_src  rows to gather from (x itself for linear; img_feat for grid_vid), gather_rows rows
 *   out_rows    T[cap, D]; idx_out int64[cap]; ks int64[F]; K_out int64[2] (see vc2_select)
 *   v_T/f_T     optional T[F,N] score outputs (NULL to skip)
 */
int vc2_compress(const void* x, int64_t F, int64_t N, int64_t D, int dtype, double base_scale,
                 int map_mode, int64_t grid_h, const void* gather_src, int64_t gather_rows,
                 void* ws, size_t ws_bytes, void* out_rows, int64_t* idx_out, int64_t cap,
                 int64_t* ks, int64_t* K_out, void* v_T, void* f_T, void* stream);

/* The same pass with
 *  - `tail_rows` extra rows (T[tail_rows, D], e.g. LLaVA's image_newline embedding, reference
 *    models/llava.py:160-168) written right behind the K kept rows by the gather launch itself: out_rows is
 *    T[cap + tail_rows, D] and rows [0, K + tail_rows) are valid afterwards;
 *  - flags & VC2_FLAG_HAVE_STATS: sweep 1 is skipped -- ws already holds the channel-statistics partials of x,
 *    left there by vc2_pool_stats on the same stream (same F, N, D, dtype). */
#define VC2_FLAG_HAVE_STATS 1
int vc2_compress_ex(const void* x, int64_t F, int64_t N, int64_t D, int dtype, double base_scale,
                      int map_mode, int64_t grid_h, const void* gather_src, int64_t gather_rows,
                      void* ws, size_t ws_bytes, void* out_rows, int64_t* idx_out, int64_t cap,
                      int64_t* ks, int64_t* K_out, void* v_T, void* f_T, const void* tail, int64_t tail_rows,
                      int flags, void* stream);

/* vc2_compress_ex with a HOST MIRROR of the count: K_host (NULL: none) points at FOUR int64 words of pinned, device-mapped
 * host memory (hipHostMalloc / torch's pin_memory).  The selection launch writes K_host[1] = the status known so far and
 * then K_host[0] = K_out[0] there, BEFORE the gather launch runs: a caller that sets K_host[0] = -1 beforehand and spins
 * in vc2_wait_host_count has the one number it needs on the host (the reference's `.tolist()`, vidcom2.py:72) ~15 us
 * before the pass ends and without a device-to-host copy behind it; everything it does with the outputs afterwards is
 * ordered by the stream.  K_host[1] is the EARLY status (capacity, expired waits, guard hits of the earlier kernels); the
 * last selection workgroup to finish writes K_host[2] = the launch's final status | 2^62 (set K_host[2] = 0 beforehand):
 * a caller that went on with the early words must look at K_host[2] before it relies on the kept set being what the
 * reference keeps (bit 4, a loop bound of the selection replay expired: "cannot happen", never swallowed).
 * vc2_wait_host_count returns the count, or a negative number after timeout_s seconds. */
int vc2_compress_ex2(const void* x, int64_t F, int64_t N, int64_t D, int dtype, double base_scale,
                     int map_mode, int64_t grid_h, const void* gather_src, int64_t gather_rows,
                     void* ws, size_t ws_bytes, void* out_rows, int64_t* idx_out, int64_t cap, int64_t* ks,
                     int64_t* K_out, void* v_T, void* f_T, const void* tail, int64_t tail_rows, int flags,
                     int64_t* K_host, void* stream);
int64_t vc2_wait_host_count(const int64_t* K_host, double timeout_s);

/* vc2_compress_ex2 with the method's three hyper-parameters besides the retention ratio.  params == NULL: the reference's
 * defaults -- vc2_compress_ex2 forwards here with NULL -- and a set EQUAL to them (int(D * 0.5) channels, temp 0.01, the
 * five scales 2^-3 .. 2^1 in order) is the same pass: the same kernel instantiations, launches and bits.
 *   channels  C = int(D * ratio) of select_low_var_channels (vidcom2.py:41), computed by the caller the way Python does;
 *             1 <= C <= min(D, 4096).  C == D takes the two-launch variance + selection form; C != D / 2 takes the
 *             row-interleaved sweep 2 (the streamlined and torch-ordered forms are built for C = D / 2).
 *   temp      compute_scales' temp (vidcom2.py:66); finite, > 0
 *   alphas    _multi_scale_gaussian's scales (vidcom2.py:54, :59-62) in LIST order, the order Python's sum() adds the
 *             terms; each finite and > 0; 1..16 of them.  Scales other than the reference's five go BY VALUE into sweep
 *             3's epilogue, which then computes like vc2_multi_scale_gaussian: two_a = float(2.0 * a), the quotient
 *             correctly rounded, every term rounded to T, v_exp_f32 where it provably rounds like the fp64 exp
 *             (|arg| <= 16 and not boundary-near), the fp64 exp elsewhere.
 * channels < 1 or > D, a non-positive or non-finite temp or scale, n_alphas < 1: VC2_ERR_ARG; channels > 4096 or
 * n_alphas > 16: VC2_ERR_UNSUPPORTED; nothing is enqueued.  The workspace of vc2_workspace_bytes serves every set; every
 * numerics mode, VC2_FLAG_HAVE_STATS, tail_rows, the host mirror and both mappings work as without params.
 * The frame-sharded pass takes the same set through the `_o` forms of its entry points (vc2_shard_opts, below). */
typedef struct {
  int64_t channels;
  double temp;
  int32_t n_alphas;
  double alphas[16];
} vc2_pass_params;
int vc2_compress_ex3(const void* x, int64_t F, int64_t N, int64_t D, int dtype, double base_scale,
                     int map_mode, int64_t grid_h, const void* gather_src, int64_t gather_rows,
                     void* ws, size_t ws_bytes, void* out_rows, int64_t* idx_out, int64_t cap, int64_t* ks,
                     int64_t* K_out, void* v_T, void* f_T, const void* tail, int64_t tail_rows, int flags,
                     int64_t* K_host, const vc2_pass_params* params, void* stream);

/* vc2_compress_ex3 with the dtype the pass SCORES in, apart from the dtype x is stored in (vidcom2.py:15-36 applied to
 * the widened input x.float(), without materialising it).
 *   score_dtype == dtype                               exactly vc2_compress_ex3 (which forwards here): the same launches, the same bits
 *   score_dtype == VC2_F32, dtype VC2_BF16 / VC2_F16   the rows are loaded as 16-bit values and widened in registers; every op of
 *             the reference then rounds to fp32, as in the pass over fp32 inputs: fp64 reductions, F.normalize's eps as the
 *             fp32 1e-12 (a zero row scores like the reference on x.float(), not NaN as native fp16 does), the fp32 norm
 *             overflow rule, fp32 budgets, 64-bit selection words -- and no "torch order" replays: vc2_set_mode only
 *             decides what it decides for fp32 inputs.  The result stands to the reference on x.float() where the
 *             fp32-input pass stands to the reference on fp32 inputs: equal budgets, equal kept indices outside score ties
 *             below the fp32 reduction noise, scores within 1e-6.
 *   anything else                                      VC2_ERR_ARG; nothing is enqueued.
 * In the fp32-scored pass v_T / f_T, when requested, are FLOAT[F, N]; out_rows, tail and gather_src stay in `dtype` (the row
 * gather copies 16-bit rows); ks, idx_out, K_out, the host mirror words, flags (VC2_FLAG_HAVE_STATS: vc2_pool_stats' partials
 * are arithmetic-neutral fp64 sums of the stored values), params and map_mode / grid_h behave as in vc2_compress_ex3.  Row-width
 * and channel limits are those of the storage dtype (D <= 8192, D % 8 == 0 for the vector path).  The workspace of
 * vc2_workspace_bytes(F, N, D, dtype) serves both passes: the fp32-scored one lays out the same arrays and needs none of
 * the replay engine's.
 * The stage entry points keep one dtype.  The frame-sharded `_o` forms take a score_dtype with these meanings and checks
 * (vc2_shard_opts below): VC2_F32 over 16-bit rows is the fp32-scored pass across ranks. */
int vc2_compress_ex4(const void* x, int64_t F, int64_t N, int64_t D, int dtype, double base_scale,
                     int map_mode, int64_t grid_h, const void* gather_src, int64_t gather_rows,
                     void* ws, size_t ws_bytes, void* out_rows, int64_t* idx_out, int64_t cap, int64_t* ks,
                     int64_t* K_out, void* v_T, void* f_T, const void* tail, int64_t tail_rows, int flags,
                     int64_t* K_host, const vc2_pass_params* params, int score_dtype, void* stream);

/* vc2_compress_ex4 with the newline vector of the grid mapping (vidcom2.py:93-96, :105-115; models/llava.py:118-127):
 * newline == NULL is exactly vc2_compress_ex4 (which forwards here).  newline = T[D] (the model's image_newline, in `dtype`)
 * requires map_mode == VC2_MAP_GRID_VID (VC2_ERR_ARG otherwise, as for N != grid_h^2): gather_src / gather_rows are then
 * ignored and the gather launch reads the kept rows from x itself and the newline rows from the vector, as
 * vc2_gather_rows_grid does -- out_rows holds the bits of img_feat[idx_out] for the img_feat add_token_per_grid would have
 * built.  idx_out stays in the stream's index space, K_out[0] still counts the F * grid_h newline rows, cap is unchanged.
 * The newline pointer needs no alignment (a misaligned one takes the scalar copy). */
int vc2_compress_ex5(const void* x, int64_t F, int64_t N, int64_t D, int dtype, double base_scale,
                     int map_mode, int64_t grid_h, const void* gather_src, int64_t gather_rows,
                     void* ws, size_t ws_bytes, void* out_rows, int64_t* idx_out, int64_t cap, int64_t* ks,
                     int64_t* K_out, void* v_T, void* f_T, const void* tail, int64_t tail_rows, int flags,
                     int64_t* K_host, const vc2_pass_params* params, int score_dtype, const void* newline,
                     void* stream);

/* ---- upstream fusion: LLaVA's get_2dPool (llava/model/llava_arch.py:171-190) + sweep 1 -------
 * xin T[F, H*W, D] (the projector output, token-major) -> x_out T[F, h*w, D] = its 2x2 pool, and the sweep-1
 * channel-statistics partials of x_out in ws (workspace of vc2_workspace_bytes(F, h*w, D)): the pooled tensor is
 * written once and vc2_compress_ex(..., VC2_FLAG_HAVE_STATS) reads it only twice more.
 *   VC2_POOL_AVG       avg_pool2d(kernel 2, stride 2): h = H/2, w = W/2; bit-exact to torch (fp32 sum in window order, / 4)
 *   VC2_POOL_MAX       max_pool2d(2): bit-exact (NaN propagates like torch)
 *   VC2_POOL_BILINEAR  interpolate(size=ceil(H/2) x ceil(W/2), mode="bilinear", align_corners=False): bit-exact to
 *                      torch 2.10's x86 CPU kernel (ATen's source index / lambda arithmetic and the fma order of its
 *                      vectorised channel loop); needs D % 8 == 0 (fp32) / D % 16 == 0 (16-bit), else
 *                      VC2_ERR_UNSUPPORTED (the loop's scalar tail contracts differently). */
#define VC2_POOL_AVG 1
#define VC2_POOL_MAX 2
#define VC2_POOL_BILINEAR 3
int vc2_pool_out_tokens(int64_t H, int64_t W, int mode, int64_t* h_out, int64_t* w_out);
int vc2_pool_stats(const void* xin, int64_t F, int64_t H, int64_t W, int64_t D, int dtype, int mode, void* ws,
                   size_t ws_bytes, void* x_out, void* stream);

/* ---- hook-side fusion: kept rows written once, at their final positions ------------
 * vc2_gather_scatter: up to 8 tensors T[src_rows[t], D] share ONE index list:
 *     dsts[t][dst_pos ? dst_pos[j] : dst_row0 + j] = srcs[t][idx ? idx[j] : j]      for j < n
 * n = min(n_dev[0], n_max) when n_dev (device) is given, else n_max; `tail_rows` rows of `tail` are appended to dsts[0]
 * behind the gathered ones (dst_row0 + n ...).  srcs / dsts / src_rows / dst_rows are HOST arrays of n_src entries.
 * Replaces flat[global_idx] + torch.cat(newline) (vidcom2.py:91, models/llava.py:160-168), inputs_embeds[:, keep]
 * (models/qwen2_5_vl.py:162-182) and the N+1 gathers of Qwen3-VL's deep-stack (models/qwen3_vl.py:140-165).
 * status (optional device word): |= 2 if a row index fell outside its tensor (such rows are skipped).
 * vc2_keep_positions (models/qwen2_5_vl.py:153-160): keep_out = ascending positions s in [0, S) with
 * !video_mask[s] or (ordinal of s among the video positions) in kept[0..K) (ascending); K = min(K_dev[0], K_max) or
 * K_max; vis_rows_out (optional, needs visual_mask) = ordinals, among the positions flagged in visual_mask, of the
 * kept ones.  keep_cap / vis_cap = entries the two outputs hold: nothing is written past them.  counts_out (optional,
 * device int64[3]) = {positions found, visual rows found, error bits}: 1 = more positions than keep_cap, 2 = more
 * visual rows than vis_cap, 4 = kept[] not strictly ascending inside [0, video positions), 8 = fewer positions than
 * keep_cap (the rest of keep_out is then filled with -1, which vc2_gather_scatter reports instead of reading). */
int vc2_gather_scatter(const void* const* srcs, const int64_t* src_rows, void* const* dsts, const int64_t* dst_rows,
                       int n_src, int64_t D, int dtype, const int64_t* idx, const int64_t* n_dev, int64_t n_max,
                       const int64_t* dst_pos, int64_t dst_row0, const void* tail, int64_t tail_rows,
                       int32_t* status, void* stream);
int vc2_keep_positions(const uint8_t* video_mask, int64_t S, const int64_t* kept, const int64_t* K_dev, int64_t K_max,
                       const uint8_t* visual_mask, int64_t* keep_out, int64_t keep_cap, int64_t* vis_rows_out,
                       int64_t vis_cap, int64_t* counts_out, void* stream);

/* ---- batched prefill pruning (B > 1 prompts of a padded batch) ---------------------------------------------------
 * Each entry batches the per-row operation of models/qwen2_5_vl.py:156-183 (keep every non-video position of a row plus
 * its kept video tokens, slice the prompt tensors to them) and re-pads the pruned rows, which now differ in length.
 *
 * vc2_keep_positions_batched: video_mask uint8[B, S]; kept[K] = the batch's kept video ordinals, strictly ascending over
 * the video positions of the whole batch in row-major order (the order of HF's video mask and of video_grid_thw).  Row b
 * keeps its n_b = S - (video positions of b) + (kept ordinals in b) positions; S' = max n_b.  Outputs, written with row
 * length S' (capacity: B * S_cap entries for keep_out / mask_out, R * B * S_cap for pos_out):
 *   keep_out int64[B, S']    kept positions of row b in order at slots [off_b, off_b + n_b), -1 in the other slots
 *                            (pad slots); off_b = S' - n_b when pad_left, else 0
 *   lengths_out int64[B]     n_b
 *   vis_rows_out (optional, needs visual_mask uint8[B, S])  ordinals, among the flattened visual positions of the batch,
 *                            of the kept ones (the rows Qwen3-VL's deep-stack tensors keep); at most vis_cap
 *   mask_out (optional, needs attention_mask int64[B, S])  attention_mask gathered at keep_out, 0 in pad slots
 *                            (attention_mask NULL: 1 in the kept slots)
 *   pos_out (optional, needs pos int64[R, B, S], R <= 4)  every plane gathered at keep_out; a pad slot holds the plane's
 *                            value at the row's first existing pad slot (attention_mask == 0), 0 when the row has none.
 *                            Without text_row0 the values are only copied, never computed on: any 64-bit payload
 *                            (e.g. the bits of fp64 positions, whose 0.0 is the all-zero word) comes back exactly.
 *                            text_row0: plane 0 holds text positions instead -- in a kept slot with attention_mask != 0
 *                            its rank among those slots of the row (0, 1, ...), in the other slots the pad value.
 * row_ws: device scratch of 4 * B int64.  counts_out (optional; device memory, or pinned host memory that is then stored
 * system-scope, the error word last, for a host spinning on counts_out[2] preset to -1) = {S', kept visual rows, error
 * bits}: 1 = S' > S_cap, 2 = more visual rows than vis_cap, 4 = kept[] not strictly ascending inside [0, video positions
 * of the batch), 8 = the batch's video positions differ from n_video (n_video < 0: not checked), 16 = a video position
 * the visual mask does not flag.  On any error nothing but lengths_out (zeros) and counts_out is written.
 * Two launches (per-row statistics, then the rows), no host round trip.  B <= 256, S <= 983 040.
 *
 * vc2_repad_rows: dst[b, j, :] = src[b, keep[b, j], :] for src T[B, S, D], keep int64[B, Sp] (vc2_keep_positions_batched's
 * keep_out), dst T[B, Sp, D]; a zero row where keep[b, j] < 0.  An entry >= S is not read: its row is zeroed and
 * status (optional device word) |= 2. */
int vc2_keep_positions_batched(const uint8_t* video_mask, int64_t B, int64_t S, const int64_t* kept, int64_t K,
                               int64_t n_video, int pad_left, const uint8_t* visual_mask, const int64_t* attention_mask,
                               const int64_t* pos, int64_t R, int text_row0, int64_t* keep_out, int64_t* lengths_out,
                               int64_t S_cap, int64_t* vis_rows_out, int64_t vis_cap, int64_t* mask_out, int64_t* pos_out,
                               int64_t* row_ws, int64_t* counts_out, void* stream);
int vc2_repad_rows(const void* src, int64_t B, int64_t S, int64_t D, int dtype, const int64_t* keep, int64_t Sp, void* dst,
                   int32_t* status, void* stream);

/* ---- backward of the gathers (vidcom2_amd/autograd.py) -----------------------------------------------------------
 * Both reproduce torch's backward of x[idx] / x[:, idx] -- zeros_like(x).index_put_(idx, g, accumulate=True) -- bit for
 * bit for unique indices: a kept element comes back as 0 + g in fp32 rounded to T (-0.0 -> +0.0, a bf16 NaN -> 0x7FC0),
 * every other element is +0.0.  Every output element is written exactly once (no zero-fill pass).
 *
 * vc2_rows_grad: backward of vc2_gather_rows / vc2_gather_scatter (fresh destinations) / the gather of vc2_compress* /
 * vc2_repad_rows.  For each of n_src tensors (HOST arrays, as vc2_gather_scatter):
 *     gsrcs[t][idx ? idx[j] : j] = gdsts[t][dst_row0 + j]   for j < n,  every other row of gsrcs[t] = 0
 * n = min(n_dev[0], n_max) when n_dev (device) is given, else n_max; gdsts[t] holds gdst_rows[t] >= dst_row0 + n_max rows,
 * gsrcs[t] gsrc_rows[t].  Entries idx[j] < 0 are skipped (pad slots).  idx given: inv_ws = device scratch of inv_len >=
 * max(gsrc_rows) int32 (the inverse map: one memset, one launch), then one streaming launch.  status (optional device
 * word) |= 1 for a duplicate index (the row then holds ONE of its gradients: the caller must fall back to an
 * accumulating scatter), |= 2 for an index >= max(gsrc_rows) (skipped).
 *
 * vc2_cols_grad: backward of vc2_gather_cols: gx T[R, D], gx[r, idx[c]] = g[r, c] for c < C, zero elsewhere; g T[R, C].
 * D <= 8192 (the channel inverse map lives in LDS).  status (optional) |= 1 duplicate column, |= 2 column outside [0, D). */
int vc2_rows_grad(const void* const* gdsts, const int64_t* gdst_rows, void* const* gsrcs, const int64_t* gsrc_rows,
                  int n_src, int64_t D, int dtype, const int64_t* idx, const int64_t* n_dev, int64_t n_max,
                  int64_t dst_row0, int32_t* inv_ws, int64_t inv_len, int32_t* status, void* stream);
int vc2_cols_grad(const void* g, int64_t R, int64_t C, int64_t D, int dtype, const int64_t* idx, void* gx,
                  int32_t* status, void* stream);

/* ---- frame-sharded multi-GPU building blocks -------------------------
 * A rank holds frames [f0, f0+F_local) of a video with F_total frames.  Between the local sweeps the Python
 * layer all-gathers three small fp64 / fp32 arrays over RCCL.  Exchanges 1 and 2 carry CANONICAL partials -- per
 * stat block of 8 frames (mean, M2), per group of 16 frames the sums of the normalised tokens -- that every rank then
 * folds in the same fixed order, so the reduced bits do not depend on the world size or on how the frames are split
 * (ranks holding a multiple of 16 frames each, equal or not; otherwise equal up to fp64 rounding):
 *   1. per stat block (mean, M2)   bstats[nb][2][D], nb = F_local / block_frames     -> vc2_chan_var_from_stats
 *   2. per 16-frame group: sums of x^, then bounds of sum |x^|   csum_parts[2 * ceil(F_local/16)][C]   -> vc2_scores_phase2
 *      (the bounds size the video centre's replay margin soundly, see mean_delta in the kernels)
 *   3. per-frame uniqueness   s[F_local]                                               -> vc2_select_sharded
 * F_total (the WHOLE video's frame count) fixes how frames are cut into row groups / splits on every rank. */
int vc2_stat_block_frames(void);     /* 8: the unsharded pass's stat block */
/* block_frames: frames per stat block, 1..8; use 8 when every rank's F_local is a multiple of 8 (bit-identical to the
 * unsharded pass), else the largest power of two dividing every rank's F_local -- the same value on every rank. */
int vc2_chan_stats(const void* x, int64_t F, int64_t N, int64_t D, int dtype, int64_t F_total, int block_frames,
                   void* ws, size_t ws_bytes, double* bstats /*[F / block_frames][2][D]*/, void* stream);
/* bstats of ALL ranks concatenated in rank order; rows_per_block = block_frames * N (the last block holds the
 * remainder). */
int vc2_chan_var_from_stats(const double* bstats /*[NB][2][D]*/, int64_t NB, int64_t rows_per_block,
                            int64_t R_total, int64_t D, int dtype, void* var_T, float* var_f32, void* stream);
/* perm != NULL (with var_f32 = the widened variances vc2_chan_select consumed): in mode 1 spos[C] is PRODUCED by a
 * rider workgroup of sweep 2 (the ORDER replay of vc2_chan_select, off the critical path) and then used by the
 * fix-up kernels; perm == NULL: spos must already be valid (or NULL: mode 0 / cols == NULL). */
int vc2_scores_phase1(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                      int64_t C, int32_t* spos, const int32_t* perm, const float* var_f32, int64_t F_total,
                      void* ws, size_t ws_bytes, double* csum_parts /*[2 * ceil(F/16)][C]*/, void* stream);
/* csum_all: the ranks' csum_parts in rank order, P rows in all; rows_per_rank = rows every rank contributed
 * (2 * ceil(F_local/16): sums, then bounds), or 0 for sums only (then |x^| <= 1 bounds the margin: sound, but many
 * more columns are treated as boundary-near). */
int vc2_scores_phase2(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                      int64_t C, const int32_t* spos, const double* csum_all /*[P][csum_stride]*/, int64_t P,
                      int64_t csum_stride, int64_t rows_per_rank, int64_t R_total, void* ws, size_t ws_bytes, void* v_T,
                      void* f_T, float* total_f32, float* s_f32, void* stream);
/* Video-centre replay of the frame-sharded pass ("torch order" mode, 16-bit inputs, every rank the same number of
 * rows -- ranks with unequal row counts: the _ragged forms below -- and at least B of them, B = 16 rows up to 2^19 tokens per video, 32 up to 2^23, 64 up to 2^25 -- torch's
 * level_power 4 / 5 / 6).  Between exchange 2 and phase 2:
 *   vc2_video_centre_blocks  flags the boundary-near video-centre columns (identically on every rank) and writes, for
 *                            the first `cap` of them, a record of 129 + F*N/16 floats to blocks_out[cap][129 + F*N/16]:
 *                            [0,64) the x^ values of this rank's first rows that end a B-row block begun by the previous
 *                            rank (row0 = the video row index of this rank's first row tells how many), [64,128) those
 *                            of its last rows that begin a block the next rank ends, [128,..) the sums of its complete
 *                            blocks (rows added in order: torch's SumKernel cascade, level 0)
 *   (all-gather -> blocks_all[world][cap][129 + F*N/16], rank order)
 *   vc2_scores_phase2_blocks = vc2_scores_phase2, which then finishes the cascade over the whole video for those
 *                            columns, so their means round like the unsharded pass / the reference.
 * When the conditions do not hold both calls fall back to vc2_scores_phase2's behaviour (exact means, counted). */
int vc2_video_centre_blocks(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                            int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                            int64_t csum_stride, int64_t rows_per_rank, int64_t R_total, int64_t row0, void* ws,
                            size_t ws_bytes, float* blocks_out, int cap, void* stream);
int vc2_scores_phase2_blocks(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                             int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                             int64_t csum_stride, int64_t rows_per_rank, int64_t R_total, void* ws, size_t ws_bytes,
                             void* v_T, void* f_T, float* total_f32, float* s_f32, const float* blocks_all, int world,
                             int cap, void* stream);

/* More flagged columns than one exchange carries (only the proven-margin and debug modes flag that many): further
 * ROUNDS of exchange 2b.  After vc2_video_centre_blocks (round 0: flags, count, records of the first `cap` columns) the
 * caller reads the count (vc2_video_centre_flagged; every rank reads the same number), and for every round r:
 *   vc2_video_centre_blocks_round(col_offset = r * cap)   records of flagged columns [r * cap, (r + 1) * cap)   (r >= 1)
 *   (all-gather)
 *   vc2_video_centre_finish_round(col_offset = r * cap)   torch's cascade over the whole video for those columns; the
 *                                                         video centre in the workspace is corrected in place  (r >= 0)
 * and finally vc2_scores_phase2_blocks(blocks_all = NULL, world = -1): "the centre is final", sweep 3 only.
 * A level-0 block may meet any number of ranks (ranks with fewer rows than a block included); the ranks must hold
 * equal row counts (unequal ones: the _ragged forms below). */
int vc2_video_centre_blocks_round(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                  int64_t C, const int32_t* spos, int64_t R_total, int64_t row0, void* ws,
                                  size_t ws_bytes, float* blocks_out, int cap, int col_offset, void* stream);
int vc2_video_centre_flagged(int64_t F, int64_t N, int64_t D, int dtype, int64_t R_total, const void* ws, size_t ws_bytes,
                             int32_t* count_host, void* stream);   /* synchronises `stream`; host pointer */
int vc2_video_centre_finish_round(int64_t F, int64_t N, int64_t D, int dtype, int64_t C, const int32_t* spos,
                                  int64_t R_total, void* ws, size_t ws_bytes, const float* blocks_all, int world,
                                  int cap, int col_offset, void* stream);

/* Exchange 2b for ranks with UNEQUAL row counts.  The _ragged forms take the layout of the video over the ranks instead of
 * assuming R_total == world * F * N: `world`, this rank's `rank`, and the HOST array rank_rows[world] (rows = frames * N of
 * every rank in rank order; their sum is R_total, every entry >= N -- no empty rank --, rank_rows[rank] == F * N).  From it
 * they take this rank's row0 (the prefix sum) and ONE record stride for all ranks, 129 + max(rank_rows) / 16 floats, so
 * that the all-gather stays rectangular: blocks_out[cap][stride], blocks_all[world][cap][stride].  A record's layout, the
 * flags, the rounds and the arithmetic are those of the equal-rank forms (a straddling block is its rows' raw values added
 * in row order, from however many ranks it meets; complete blocks come from the records); the owner of a video row is
 * found in the prefix sums of rank_rows, which reach the kernel by value (no copy, no synchronisation).  At most
 * VC2_RAGGED_MAX_WORLD ranks; more give VC2_ERR_UNSUPPORTED.  The other sharded entry points need no ragged form:
 * they take (f0, F, F_total) or block counts as they are.  What the caller lays out (vidcom2_amd/sharded.py does):
 *   exchange 1  block_frames = the largest power of two <= 8 dividing EVERY rank's frame count, the ranks' blocks
 *               compacted to bstats[sum nb_p][2][D] in rank order -- one uniform grid of the video
 *   exchange 2  a rank with fewer 16-frame groups than the largest pads INSIDE each half of its csum_parts block (zero
 *               sums, zero bounds: rows_per_rank = 2 * the largest group count); zeros change neither sums nor bounds
 * vc2_scores_phase2_blocks_ragged always finishes the cascade (blocks_all must be the gathered records); "the centre is
 * final" (world = -1) and "no records" stay with vc2_scores_phase2_blocks, which does not look at the layout then. */
#define VC2_RAGGED_MAX_WORLD 64
int vc2_video_centre_blocks_ragged(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                   int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                                   int64_t csum_stride, int64_t rows_per_rank, int64_t R_total,
                                   const int64_t* rank_rows /* host [world] */, int world, int rank, void* ws,
                                   size_t ws_bytes, float* blocks_out, int cap, void* stream);
int vc2_video_centre_blocks_round_ragged(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                         int64_t C, const int32_t* spos, int64_t R_total,
                                         const int64_t* rank_rows /* host [world] */, int world, int rank, void* ws,
                                         size_t ws_bytes, float* blocks_out, int cap, int col_offset, void* stream);
int vc2_video_centre_finish_round_ragged(int64_t F, int64_t N, int64_t D, int dtype, int64_t C, const int32_t* spos,
                                         int64_t R_total, const int64_t* rank_rows /* host [world] */, int world,
                                         int rank, void* ws, size_t ws_bytes, const float* blocks_all, int cap,
                                         int col_offset, void* stream);
int vc2_scores_phase2_blocks_ragged(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                    int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                                    int64_t csum_stride, int64_t rows_per_rank, int64_t R_total,
                                    const int64_t* rank_rows /* host [world] */, int world, int rank, void* ws,
                                    size_t ws_bytes, void* v_T, void* f_T, float* total_f32, float* s_f32,
                                    const float* blocks_all, int cap, void* stream);

/* Step 3 of the sharded path: s_all_f32[F_total] = the all-gathered per-frame uniqueness scores
 * (fp32-widened T values); budgets are computed over all F_total frames, selection + gather only for
 * this rank's frames [f0, f0+F_local).  idx_out holds LOCAL linear indices (f_local*N + n).  K_out is int64[3] here:
 * K_out[2] = the number of video-centre values within the replay margin of a T rounding boundary that exchange 2b did
 * not replay: they keep the exactly rounded mean (more flagged columns than `cap` in a mode without rounds; tail columns
 * in the narrow record layout, see vc2_shard_opts). */
int vc2_select_sharded(const float* total_f32, const float* s_all_f32, int64_t F_total, int64_t f0,
                       int64_t F_local, int64_t N, int64_t D, double base_scale, int dtype, void* ws,
                       size_t ws_bytes, int64_t* ks, int64_t* idx_out, int64_t cap, int64_t* K_out,
                       const void* gather_src, void* out_rows, void* stream);

/* ---- the frame-sharded pass with options: the `_o` forms ---------------------------------------------------------
 * Every sharded entry point that lays out the workspace or launches a parametrised kernel has a form with one trailing
 * argument, `const vc2_shard_opts* opts`.  opts == NULL is the plain symbol (which forwards here with NULL): the same
 * launches, arguments, record format and bits.  All `_o` calls of one pass, on every rank, must carry the same options.
 *   params        the pass's hyper-parameters, as in vc2_compress_ex3: the same checks and error codes, before anything is
 *                 enqueued (VC2_ERR_ARG / VC2_ERR_UNSUPPORTED; an entry point that takes C also refuses C !=
 *                 params->channels).  channels is the k of vc2_chan_select and the C of phase 1 / phase 2 / the video-centre
 *                 calls (C != D / 2: the row-interleaved sweep 2; C == D works; C > 4096 is refused); alphas go by value
 *                 into sweep 3's epilogue from the phase-2 forms (a set equal to the reference's five: the compile-time
 *                 path); temp is vc2_select_sharded_o's softmax temperature.  NULL or a set equal to the defaults: the
 *                 default pass.
 *   score_dtype   a public dtype code (0..2), checked as in vc2_compress_ex4 (anything but dtype itself, or VC2_F32 over
 *                 VC2_BF16 / VC2_F16 rows: VC2_ERR_ARG).  VC2_F32 over 16-bit rows: x, gather_src and out_rows stay 16-bit,
 *                 every kernel that reads rows loads them as stored and computes in fp32; total_f32 / s_f32 and the
 *                 selection are the fp32-input pass's.  The caller reduces the exchanged block statistics with
 *                 vc2_chan_var_from_stats(..., VC2_F32, ...): fp32 variances, which vc2_chan_select ranks through its 64-bit
 *                 selection words.  There is no "torch order" replay in fp32 arithmetic: the vc2_video_centre_* forms
 *                 enqueue nothing and K_out[2] is 0; exchanges 1-3 keep their fp64 / fp32 formats.  The workspace of
 *                 vc2_workspace_bytes(F, N, D, dtype) serves this pass too.
 *   tail_records  0: exchange 2b in the narrow record layout of vc2_video_centre_blocks (edge 64); video-centre columns in
 *                 the C % 32 tail keep their exactly rounded mean and stay counted in K_out[2].
 *                 1: the WIDE layout, which also replays the tail columns.  A tail column is one whose position in
 *                 torch.topk's order (spos) is at or above (C / 32) * 32 -- (C / 4) * 4 when C < 8.  torch sums it with
 *                 row_sum's four interleaved chains: chain k (0..3) is the cascade over the R_total / 4 values at video rows
 *                 k + 4e with level power lp4 = level_power(R_total / 4), B4 = 2^lp4; the sum is chain0, + the R_total % 4
 *                 leftover rows one by one, + chain1 + chain2 + chain3.  A level-0 block of a chain is the rows k + 4u of one
 *                 aligned RUN of 4 * B4 video rows.  Record of one flagged column, 2 * 256 + R / 16 + 1 floats (R = F * N;
 *                 ragged forms: the largest rank's rows), for plain and tail columns alike:
 *                   [0, 256)    the x^ values of this rank's first h rows: the end of a block (plain column, h < B) or of a
 *                               run (tail column, h < 4 * B4 <= 256) that began before this rank; row order
 *                   [256, 512)  the x^ values of its last t rows: the beginning of a block / run that ends after it
 *                   [512, ..)   plain column: the sums of its complete blocks.  Tail column: for every run it holds
 *                               completely four sums, one per chain, rows added in row order (stride 4): [4 * run + k]
 *                 The video's last R_total mod (4 * B4) rows (the chains' leftover elements, the R_total % 4 leftover rows)
 *                 lie in no complete run and arrive raw.  The finish kernels run the four cascades over the gathered
 *                 records, a straddling run's rows one by one from however many ranks it meets, combine them in the order
 *                 above, write the mean and take the column off the count.  Equal and ragged layouts, rounds included.
 * One vc2_workspace_bytes(F, N, D, dtype) workspace serves every combination.  vc2_chan_var_from_stats, vc2_chan_select
 * and vc2_video_centre_flagged need no `_o` form. */
typedef struct {
  const vc2_pass_params* params;
  int32_t score_dtype;
  int32_t tail_records;
} vc2_shard_opts;
int vc2_chan_stats_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, int64_t F_total, int block_frames,
                     void* ws, size_t ws_bytes, double* bstats, void* stream, const vc2_shard_opts* opts);
int vc2_scores_phase1_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                        int64_t C, int32_t* spos, const int32_t* perm, const float* var_f32, int64_t F_total,
                        void* ws, size_t ws_bytes, double* csum_parts, void* stream, const vc2_shard_opts* opts);
int vc2_video_centre_blocks_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                              int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                              int64_t csum_stride, int64_t rows_per_rank, int64_t R_total, int64_t row0, void* ws,
                              size_t ws_bytes, float* blocks_out, int cap, void* stream, const vc2_shard_opts* opts);
int vc2_scores_phase2_blocks_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                               int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                               int64_t csum_stride, int64_t rows_per_rank, int64_t R_total, void* ws, size_t ws_bytes,
                               void* v_T, void* f_T, float* total_f32, float* s_f32, const float* blocks_all, int world,
                               int cap, void* stream, const vc2_shard_opts* opts);
int vc2_video_centre_blocks_round_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                    int64_t C, const int32_t* spos, int64_t R_total, int64_t row0, void* ws,
                                    size_t ws_bytes, float* blocks_out, int cap, int col_offset, void* stream,
                                    const vc2_shard_opts* opts);
int vc2_video_centre_finish_round_o(int64_t F, int64_t N, int64_t D, int dtype, int64_t C, const int32_t* spos,
                                    int64_t R_total, void* ws, size_t ws_bytes, const float* blocks_all, int world,
                                    int cap, int col_offset, void* stream, const vc2_shard_opts* opts);
int vc2_video_centre_blocks_ragged_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                     int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                                     int64_t csum_stride, int64_t rows_per_rank, int64_t R_total,
                                     const int64_t* rank_rows /* host [world] */, int world, int rank, void* ws,
                                     size_t ws_bytes, float* blocks_out, int cap, void* stream,
                                     const vc2_shard_opts* opts);
int vc2_video_centre_blocks_round_ragged_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype,
                                           const int32_t* cols, int64_t C, const int32_t* spos, int64_t R_total,
                                           const int64_t* rank_rows /* host [world] */, int world, int rank, void* ws,
                                           size_t ws_bytes, float* blocks_out, int cap, int col_offset, void* stream,
                                           const vc2_shard_opts* opts);
int vc2_video_centre_finish_round_ragged_o(int64_t F, int64_t N, int64_t D, int dtype, int64_t C, const int32_t* spos,
                                           int64_t R_total, const int64_t* rank_rows /* host [world] */, int world,
                                           int rank, void* ws, size_t ws_bytes, const float* blocks_all, int cap,
                                           int col_offset, void* stream, const vc2_shard_opts* opts);
int vc2_scores_phase2_blocks_ragged_o(const void* x, int64_t F, int64_t N, int64_t D, int dtype, const int32_t* cols,
                                      int64_t C, const int32_t* spos, const double* csum_all, int64_t P,
                                      int64_t csum_stride, int64_t rows_per_rank, int64_t R_total,
                                      const int64_t* rank_rows /* host [world] */, int world, int rank, void* ws,
                                      size_t ws_bytes, void* v_T, void* f_T, float* total_f32, float* s_f32,
                                      const float* blocks_all, int cap, void* stream, const vc2_shard_opts* opts);
int vc2_select_sharded_o(const float* total_f32, const float* s_all_f32, int64_t F_total, int64_t f0,
                         int64_t F_local, int64_t N, int64_t D, double base_scale, int dtype, void* ws,
                         size_t ws_bytes, int64_t* ks, int64_t* idx_out, int64_t cap, int64_t* K_out,
                         const void* gather_src, void* out_rows, void* stream, const vc2_shard_opts* opts);

/* ---- one video held as frame chunks on ONE device (vidcom2_amd/chunked.py) -------------------------------------------
 * Every chunk is a logical rank of the frame-sharded pass above, its stage calls writing their partials into slots of
 * whole-video buffers.  vc2_select_chunks is step 3 for the whole video in one call -- vidcom2.py:70-78,89-91:
 *   budgets over all F_total frames, once; the per-frame selection of every frame from total_f32[F_total * N] and
 *   s_all_f32[F_total] (vc2_select_sharded's launches with f0 = 0, F_local = F_total); ks[F_total], idx_out (ascending
 *   indices into the virtual concatenation of the chunks, at most `cap` = the unsharded pass's capacity for F_total
 *   frames), K_out[3] as in vc2_select_sharded; then, when out_rows [cap, D] is given, the kept rows from the chunk
 *   table as vc2_gather_rows_chunks gathers them (chunks / chunk_rows / n_chunks / status as there; the chunks must hold
 *   F_total * N rows: VC2_ERR_ARG otherwise).  out_rows NULL: no gather, the table is not looked at.
 *   sel_ws      device scratch of vc2_select_chunks_ws_bytes(F_total) bytes (frame offsets, budgets)
 *   stage_ws    the workspace of ONE of the chunks' stage calls and that chunk's frame count stage_frames: K_out[2], the
 *               number of video-centre values left at the exactly rounded mean, is read from it (every chunk's phase 2
 *               holds the same count)
 * The `_o` form takes the pass's vc2_shard_opts (softmax temperature, score_dtype), NULL being the plain symbol. */
int vc2_select_chunks_ws_bytes(int64_t F_total, size_t* out_bytes);
int vc2_select_chunks(const float* total_f32, const float* s_all_f32, int64_t F_total, int64_t N, int64_t D,
                      double base_scale, int dtype, void* sel_ws, size_t sel_ws_bytes, const void* stage_ws,
                      size_t stage_ws_bytes, int64_t stage_frames, int64_t* ks, int64_t* idx_out, int64_t cap,
                      int64_t* K_out, const void* const* chunks /* host */, const int64_t* chunk_rows /* host */,
                      int n_chunks, void* out_rows, int32_t* status, void* stream);
int vc2_select_chunks_o(const float* total_f32, const float* s_all_f32, int64_t F_total, int64_t N, int64_t D,
                        double base_scale, int dtype, void* sel_ws, size_t sel_ws_bytes, const void* stage_ws,
                        size_t stage_ws_bytes, int64_t stage_frames, int64_t* ks, int64_t* idx_out, int64_t cap,
                        int64_t* K_out, const void* const* chunks /* host */, const int64_t* chunk_rows /* host */,
                        int n_chunks, void* out_rows, int32_t* status, void* stream, const vc2_shard_opts* opts);
/* vidcom2.py:70-78, :89-96, :105-115  vc2_select_chunks_o with the mapping and gather options of vc2_compress_ex5.
 * VC2_MAP_GRID_VID (grid_h * grid_h == N): idx_out is in the slot space of the [F_total*grid_h*(grid_h+1), D] stream,
 * every frame's kept tokens are followed by its grid_h newline slots and K_out[0] counts them; `cap` is then the
 * unsharded pass's capacity plus F_total * grid_h.  out_rows is [cap + tail_rows, D] and is written by
 * vc2_gather_rows_grid_chunks' kernel: kept rows from the chunk table, newline slots from `newline`, `tail_rows` rows of
 * `tail` behind row K.  VC2_ERR_ARG: another map mode, grid_h * grid_h != N under the grid mode, a newline without the grid
 * mode, the grid mode with out_rows but no newline, tail_rows < 0 or without tail; nothing is enqueued.  VC2_MAP_LINEAR
 * without newline and tail: vc2_select_chunks_o (which forwards here), its launches and its bits. */
int vc2_select_chunks_x(const float* total_f32, const float* s_all_f32, int64_t F_total, int64_t N, int64_t D,
                        double base_scale, int dtype, void* sel_ws, size_t sel_ws_bytes, const void* stage_ws,
                        size_t stage_ws_bytes, int64_t stage_frames, int64_t* ks, int64_t* idx_out, int64_t cap,
                        int64_t* K_out, const void* const* chunks /* host */, const int64_t* chunk_rows /* host */,
                        int n_chunks, void* out_rows, int32_t* status, void* stream, const vc2_shard_opts* opts,
                        int map_mode, int64_t grid_h, const void* newline, const void* tail, int64_t tail_rows);

/* llava_arch.py:171-190 + vidcom2.py:39-40 for ONE chunk of a frame-sharded / chunked video: vc2_pool_stats with the plan
 * of vc2_chan_stats_o (F_total frames in the whole video, stat blocks of block_frames frames), followed by the block
 * reduction vc2_chan_stats_o runs: x_out = the pooled chunk, bstats[F / block_frames, 2, D] = what
 * vc2_chan_stats_o(x_out, F, h*w, D, ...) would write -- the chunk's sweep 1 never runs.  ws: the chunk's stage workspace.
 * Limits and codes of vc2_pool_stats and vc2_chan_stats_o; opts as there (NULL: the plain pass). */
int vc2_pool_stats_blocks(const void* xin, int64_t F, int64_t H, int64_t W, int64_t D, int dtype, int mode,
                          int64_t F_total, int block_frames, void* ws, size_t ws_bytes, void* x_out, double* bstats,
                          void* stream, const vc2_shard_opts* opts);

/* _multi_scale_gaussian(x, center, alphas) as a standalone call -- vidcom2.py:59-62 (the fused pass
 * never materialises x; this entry serves callers of the helper itself).  x: T[F*N, C] as given,
 * centre: T[n_centres, C] with n_centres == 1 (video centre) or F (one per frame), alphas: n_alphas
 * host doubles (<= 16).  out: T[F*N] = sum_a exp(-||x - c||^2 / (2 a)), every op rounded to T. */
int vc2_multi_scale_gaussian(const void* x, int64_t F, int64_t N, int64_t C, int dtype, const void* centre,
                             int64_t n_centres, const double* alphas, int n_alphas, void* out_T, void* stream);

/* ---- small device utilities used by tests / bench ----------------------------------- */
/* exp over every T bit pattern as the path computes it: out[i] = RN_T(exp(in[i])) (KAT). */
int vc2_kat_exp(const void* in_T, int64_t n, int dtype, void* out_T, void* stream);
/* RN_T round trip of fp32 values (KAT for the conversion instructions). */
int vc2_kat_round(const float* in, int64_t n, int dtype, void* out_T, void* stream);

/* ---- per-kernel timing (bench.py roofline leg) ----------------------------------------
 * When enabled every kernel launch is bracketed by hipEvents on its own stream.
 * vc2_profile_collect synchronises on them and returns accumulated milliseconds / launch counts
 * per kernel (returns the number of kernels reported). */
int vc2_profile_enable(int on);
int vc2_profile_collect(int max_kernels, const char** names, double* total_ms, int64_t* launches);

/* Diagnostic (SYNCHRONISES the device): the "torch order" replay counters of the last pass that used `ws`
 * for this shape, out8 = host int32[8]. */
int vc2_pass_counters(int64_t F, int64_t N, int64_t D, int dtype, const void* ws, int32_t* out8_host);
/* Diagnostic (SYNCHRONISES): every loop of the selection replay is bounded; out8 = how often each bound actually
 * expired since the last reset (all zero on a healthy run; the test-suite asserts it). */
int vc2_selftest_counters(int32_t* out8_host, int reset);
/* Test hook: the selection launches that follow report a loop-bound hit (status bit 4) from the workgroup of local frame
 * `frame` (-1: off) -- how the test-suite checks that a hit in ANY workgroup of the launch reaches K_out[1] and the host
 * mirror's final word.  Process-wide; nothing is computed differently. */
int vc2_selftest_force_guard(int frame);
/* Host arithmetic only (no device call): the geometry of sweep 2's ORD form for this shape in the current mode -- the
 * workgroups that add a frame's x^ in torch's own order (vidcom2.py:51-52; k_norm_colsum2<.., ORD>, OrdGeo).  out5 = int32[cap][5]
 * rows {frame, piece, pieces of that frame, first 16-row block, blocks}, in launch order.  Returns the number of streaming
 * workgroups (0: the shape has no ORD geometry -- the row-interleaved sweep with margins and replays runs), or an error (< 0).
 * The test-suite checks that the pieces tile every frame exactly once and fit the resident workgroup slots. */
int vc2_selftest_ord_pieces(int64_t F, int64_t N, int64_t D, int dtype, int32_t* out5_host, int64_t cap);

/* Host arithmetic only (no device call): the replay margins, in fp32-ulps, that a pass over C scored channels of this
 * dtype uses in `mode` (the codes of vc2_set_mode) -- out2 = host int32[2] {norm, squared-distance sum}; {-1, -1} where
 * nothing is replayed (mode 0, fp32).  A sum whose exactly computed value lies within the margin of a T rounding boundary
 * is replayed in torch's order.  These are the parts that cover TORCH'S accumulation error; the sweeps add the bound of
 * their own fp32 accumulation on top.  With k = the roundings along the deepest path of torch's sum of C non-negative
 * terms, torch's sum is within k 2^-24 (relative) of the exact one:
 *   norm      bf16: 8 interleaved chains, k = 2 (C / 16) + 7 + C % 16; fp16: ONE sequential chain, k = C.  After the
 *             square root: k / 2 + 1 ulps.  The margin is max(128, that bound) for bf16 in every mode and for fp16 in
 *             modes 3 and 2; for fp16 in modes 4 and 1 it is 128 whatever C is -- a bound up to C = 254 only, an
 *             empirical margin beyond (what the bound would cost, and the inputs that need it).
 *   distance  SumKernel.cpp's cascade: k <= 33 up to C = 4096 (37 up to 8192), so k + 1 <= 38 ulps; the margin is 48 in
 *             every mode.
 * The test-suite derives both bounds from the oracle's summation structure and checks the margins against them. */
int vc2_selftest_margins(int64_t C, int dtype, int mode, int32_t* out2_host);

#ifdef __cplusplus
}
#endif
#endif /* VC2_H_ */
