/* fpq.h - C ABI of libfpq_hip.so: MI355X (gfx950) fake-quantization kernels that
 * replace FPQVAR's `quant_cuda` extension and the torch-op bodies of its
 * `fp_quant_*` / `fp6_quant_*` functions.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the name says `host`;
 *   - nothing allocates, nothing synchronises the host, everything is enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the null stream);
 *   - re-entrant and thread-safe: no mutable global state on any launch path.  The ONE piece of process-wide state is
 *     the table of experiment switches below (fpq_set_option): filled from the environment once, when the library is
 *     loaded, and read as plain ints afterwards - no entry point calls getenv();
 *   - returns FPQ_OK (0) or a negative FPQ_ERR_* code; on error nothing is enqueued;
 *   - rows == 0 / n == 0 is valid and enqueues nothing;
 *   - inputs are never written.
 *
 * "reference" below = PKU-SEC-Lab/FPQVAR; tr/ = models_fp_quant_transform_rotate/.
 */
#ifndef FPQ_H
#define FPQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPQ_VERSION 136 /* 0.1.2: + fpq_quant_tensor_argmin, fpq_quant_rows_segments, fpq_quant_rows_multi (round 2);
                           0.1.3: + fpq_quant_rows_codes_segments, fpq_dequant_rows_codes_segments (round 3);
                           123: + fpq_build_tag (round 4);
                           124: + fpq_set_option, fpq_get_option, fpq_option_name, fpq_gemm_fp4_gelu_dual, fpq_gelu_quant_rows_dual (round 5);
                           125: + k-major operand images: fpq_codes_to_kmajor, fpq_scales_to_kmajor, fpq_gemm_fp4_mx_km, fpq_gemm_fp4_gelu_dual_km,
                                fpq_gemm_fp6_rows_km, the *_km producers, fpq_gemm_fp4_mx_split (round 5);
                           126: - the switches FPQ_ROT_BUTTERFLY, FPQ_ADALN_V1, FPQ_ADALN_LANES, FPQ_ADALN_GRID, FPQ_BIGTAB_U
                                (the kernel forms they chose are retired);
                           127: + fpq_gemm_fp4_mx_split_qknorm, fpq_kv_cache_step_qknorm (attn_l2_norm);
                           128: + the packed KV cache: fpq_kv_pack, fpq_attention_blhc_kvcodes;
                           129: + fpq_gemm_fp6_rows_split, fpq_gemm_fp6_rows_split_qknorm (the split output and the q / k norm for W6A6);
                           130: + a format per operand on the FP6 matrix-core path (FP6 E2M3 / BF6 E3M2): fpq_quant_rows_codes_f6,
                                fpq_adaln_rotate_quant_token_rows_codes_f6, fpq_gemm_f6_rows, fpq_gemm_f6_rows_split, fpq_gemm_f6_rows_split_qknorm;
                           131: + E1M2 / E3M0 activations on the matrix cores against FP4 weights ("A6W4"): fpq_quant_rows_codes_g6,
                                fpq_gemm_a6w4_mx;
                           132: + the fc1 tail (GELU + fc2's dual-format input quantizer) in the A6W4 GEMM: fpq_gemm_a6w4_gelu_dual;
                           133: + the A6W4 path on k-major images: fpq_a6w4_quant_rows_codes_km, fpq_gemm_a6w4_mx_km, fpq_gemm_a6w4_gelu_dual_km;
                           134: + the split output and the q / k norm in the A6W4 GEMM: fpq_gemm_a6w4_mx_split, fpq_gemm_a6w4_mx_split_qknorm;
                           135: + the rotate and adaLN producers emitting the A6W4 GEMM's activation operands: fpq_a6w4_rotate_quant_rows_codes,
                                fpq_a6w4_adaln_rotate_quant_rows_codes;
                           136: + the format search's loss in one pass: fpq_sqerr_rows_weighted;
                           (136 still: + FPQ_GEMM_CFG 40, the FP4 GEMM's deep-ring small-M tiling, and fpq_gemm_fp4_tiling - an addition that changes no
                                existing entry point; a caller that wants the query looks the symbol up;
                                 + fpq_gemm_w6_mx, E1M2 / E3M0 WEIGHTS on the matrix cores as 6-bit codes against any FP4 activation format - again an
                                addition only, and the number stays because tests/test_format_search_fused_host.py pins it: look the symbol up;
                                 + its fc1 tail and split output, and all four forms on k-major images (fpq_gemm_w6_*_km): additions again;
                                 + the rotate and adaLN producers on the full FP6 tables: fpq_gf6_rotate_quant_rows_codes,
                                fpq_gf6_adaln_rotate_quant_rows_codes - additions again;
                                 + the gated residual folded into the adaLN producer behind it: fpq_resid_adaln_rotate_quant_rows, _rows_codes_mx,
                                _token_rows, _token_rows_codes_f6 - additions again) */

typedef void* fpq_stream_t; /* hipStream_t */

enum fpq_status {
  FPQ_OK = 0,
  FPQ_ERR_ARG = -1,    /* NULL pointer, negative size */
  FPQ_ERR_DTYPE = -2,  /* dtype not supported by this entry point */
  FPQ_ERR_SHAPE = -3,  /* cols == 0, k out of range, ... */
  FPQ_ERR_TABLE = -4,  /* unknown table id / half table used as symmetric table */
  FPQ_ERR_LAUNCH = -5, /* hipLaunch reported an error */
  FPQ_ERR_NO_DEVICE = -6
};

enum fpq_dtype { FPQ_F16 = 0, FPQ_F32 = 1, FPQ_F64 = 2 };

/* Built-in value tables, literal in the reference at
 * tr/quant_utils.py:233-235 (E3M0/E2M1/E1M2), :458-486 (E2M3/E3M2, two zeros),
 * :418-419 (E1M2_NEG/E2M1_POS), :488-500 (INT_NEG/E2M3_POS). */
enum fpq_table {
  FPQ_E2M1 = 0,
  FPQ_E1M2 = 1,
  FPQ_E3M0 = 2,
  FPQ_E2M3 = 3,
  FPQ_E3M2 = 4,
  FPQ_E1M2_NEG = 5,
  FPQ_E2M1_POS = 6,
  FPQ_INT_NEG = 7,
  FPQ_E2M3_POS = 8,
  FPQ_E2M1_NEG = 9, /* [-6 .. 0]: negative half of fp4_afpq_per_group_cuda, models_fp_quant/quant_utils.py:501 */
  FPQ_NUM_TABLES = 10
};

int fpq_version(void);
const char* fpq_strerror(int status);
/* Which build this is: "stock" for the shipped library, the name given to tools/build_variant.sh for a diagnostic
 * build (-DFPQ_BUILD_TAG).  The A/B tools assert on it so that a timing is never attributed to the wrong library. */
const char* fpq_build_tag(void);

/* Experiment switches - tests and the A/B tools only; a deployment never touches them.  Every switch is an int named
 * like the environment variable that initialises it: the flags FPQ_NO_HW4, FPQ_NO_HW6, FPQ_NO_FAST32, FPQ_ADALN_NO_PAIR2,
 * FPQ_ADALN_NO_TIGHT, FPQ_NO_WAVE_ROWS and the numbers FPQ_GEMM_CFG, FPQ_GEMM6_CFG, FPQ_GEMM8_CFG, FPQ_ROT_WGS,
 * FPQ_ADALN_ROWS, FPQ_ADALN_TAIL, FPQ_BIGTAB_RPB, FPQ_BIGTAB_CAP (fpq_option_name enumerates them).  The environment is read ONCE, by the library's initialiser (a variable that is set and not empty: flags take
 * 1 unless the text is "0", numbers take atoi of the text); later changes of the environment are not seen.
 * fpq_set_option changes a switch for every later call in the process (value FPQ_OPTION_DEFAULT = back to the built-in
 * choice); it is a relaxed atomic store - call it between launches, not concurrently with them, if the outcome matters.
 * Both return FPQ_ERR_ARG for an unknown name. */
#define FPQ_OPTION_DEFAULT (-2147483647 - 1)
int fpq_set_option(const char* name, int value);
int fpq_get_option(const char* name, int* value_out);
const char* fpq_option_name(int index); /* NULL past the last one */

/* Host-side copy of a built-in table exactly as the reference spells it
 * (ascending, duplicate zeros kept).  Returns the entry count, or FPQ_ERR_TABLE.
 * `host_out` may be NULL to query the size. */
int fpq_table_values(int table_id, float* host_out);

/* ---- L0: the reference's one native symbol ---------------------------------
 * Replaces quant_forward_cuda / quant_forward_cuda_kernel
 * (quant/quant_kernel.cu:11-62, bound as `quant_cuda.quant` at quant/quant.cpp:27-29).
 *   z[i] = table[j*], j* = LAST j in 0..k-1 minimising fabsf((float)x[i] - table[j])
 *   among distances <= 102400.0f; z[i] = +0.0 if there is none (NaN, +-Inf, far).
 * x, z: `dtype` in {FPQ_F32, FPQ_F64} (f64 compared in f32, as the reference does),
 * n elements, contiguous.  table: k floats on the device, 1 <= k <= 256.
 * The reference's second output (`tensor_idx`, never written, all zeros) is the
 * caller's business: the Python binding returns a zero tensor for it. */
int fpq_quant_nearest(const void* x, const float* table, void* z, int64_t n, int k, int dtype,
                      fpq_stream_t stream);

/* quantize_to_nearest_grid (tr/quant_utils.py:209-230; also the GALT / format-search scripts' copy): the lookup of
 * the reference's pure-torch path for ANY table - z[i] = table[argmin_j |(float)x[i] - table[j]|], FIRST minimal
 * index (the earlier entry on a tie), table[0] for a NaN or +-Inf input; x F16 or F32, z always float32. */
int fpq_quant_nearest_argmin(const void* x, const float* table, float* z, int64_t n, int k, int dtype,
                             fpq_stream_t stream);

/* Same lookup against a BUILT-IN table through the closed form the fused kernels
 * use (midpoint counting on the minifloat structure).  f32 only.  Exposed so
 * tests can compare it with fpq_quant_nearest element by element. */
int fpq_quant_nearest_builtin(const float* x, float* z, int64_t n, int table_id, fpq_stream_t stream);

/* ---- L1: one launch per reference function ---------------------------------
 * x: [rows, cols] contiguous, in_dtype in {F16, F32}.  out: same shape, out_dtype.
 * One scale per row of `cols` elements:
 *     s   = (T)(max|x_row| / max|table|)          (in x's dtype T)
 *     xn  = (T)(x / s)                            (in T)
 *     q   = nearest((float)xn)                    (L0 semantics)
 *     out = (Tout)((float)q * (float)s)           (fp32 product, then cast)
 * - per-group functions call it with cols = group_size (128) and rows = numel/128:
 *     fp_quant_e{1,2,3}_per_group_cuda  tr/quant_utils.py:265-282,313-330,361-378
 *     fp6_quant_{e2m3,e3m2}_per_group_cuda  :537-574   (out_dtype = F16)
 *     KV cache, kv_bit 4                tr/basic_var.py:50-67,197-198
 * - per-token functions call it with cols = last dim:
 *     fp6_quant_{e2m3,e3m2}_per_token_cuda  tr/quant_utils.py:503-534 (out_dtype = F16)
 *     KV cache, kv_bit 6 (cols = 64)    tr/basic_var.py:71-85,194-195
 * table_id must be one of the symmetric tables (E2M1, E1M2, E3M0, E2M3, E3M2). */
int fpq_quant_rows(const void* x, void* out, int64_t rows, int64_t cols, int table_id, int in_dtype,
                   int out_dtype, fpq_stream_t stream);

/* out = softmax(q k^T * scale) v per (batch, head) for head_dim 64, fp16, in the [B, L, H, c] layout the reference
 * passes to flash_attn_func(q, k, v, softmax_scale=self.scale) in SelfAttention.forward (tr/basic_var.py:173,211) -
 * the consumer of the KV cache; at inference there is no mask and no dropout (attn_bias is None with KV caching,
 * :159).  q [B, lq, H, 64] and k / v [B, lkv, H, 64] may be views: rows of H * 64 halves contiguous, batch / token
 * pitch in elements (multiples of 8) free (q out of the fused qkv output, k / v out of fpq_kv_cache_step's cache);
 * out [B, lq, H, 64] contiguous; all 16-byte aligned.  Tokens at or past lkv and anything outside the views are never
 * read: loads past the end clamp to token lkv - 1 and those keys are masked.  fp32 scores and accumulation on the
 * matrix cores, online softmax, P rounded to fp16 before P V (as in flash attention), not bit-exact.  Against the
 * float64 ref = softmax(s) v, s = scale q k^T from the fp16 inputs, with A = softmax(s) |v| and Z = sum_j exp(s_j - max s),
 * every element satisfies (for |scale q.k| <= 100)
 *     |out - ref| <= (2^-11 + 2^-13) (|ref| + A) + 2^-25 sum_j |v_jc| / Z + 2^-25
 * (output rounding, P rounding, fp32 arithmetic, fp16-subnormal P and output; derived in tests/attention_model.py). */
int fpq_attention_blhc(const void* q, const void* k, const void* v, void* out, int64_t batch, int64_t lq, int64_t lkv,
                       int64_t heads, int64_t head_dim, int64_t q_batch_pitch, int64_t q_token_pitch,
                       int64_t kv_batch_pitch, int64_t kv_token_pitch, float scale, fpq_stream_t stream);

/* One step of an incrementally maintained KV cache.  The reference
 * (SelfAttention.forward, tr/basic_var.py:186-209) re-quantizes the WHOLE cached K and V at every
 * step before concatenating the new k / v; since the quantizer returns its own output unchanged
 * (tests/test_kv_idempotence.py), only the entries appended by the previous step change.  This
 * call does both halves of a step in one launch:
 *   - fake-quantizes tokens [quant_start, quant_stop) of K and V in place, rows of `group`
 *     consecutive halves sharing one scale (64 = fp6_quant_e2m3_per_token_cuda on head_dim 64,
 *     tr/quant_utils.py:503-517; 128 = fp_quant_e2_per_group_cuda, :313-330), and
 *   - copies the new rows new_k / new_v [batch, n_new, row_elems] to tokens
 *     [new_start, new_start + n_new); their rows must be contiguous, batch and token pitch (in
 *     elements, multiples of 8) are free - views of a fused qkv projection need no copy.
 * cache: fp16 [2 (K, V), batch, max_len, row_elems], 16-byte aligned like new_k / new_v.
 * Requires quant_stop <= new_start and new_start + n_new <= max_len. */
int fpq_kv_cache_step(void* cache, int64_t batch, int64_t max_len, int64_t row_elems, int64_t quant_start,
                      int64_t quant_stop, const void* new_k, const void* new_v, int64_t new_batch_pitch,
                      int64_t new_token_pitch, int64_t new_start, int64_t n_new, int64_t group, int table_id,
                      fpq_stream_t stream);

/* THE PACKED KV CACHE: the cache fpq_kv_cache_step keeps as fake-quantized fp16, stored as the codes it holds (50 or 33 bytes per
 * (token, head) row of 64 channels instead of 128).  Layout, per kv_bit:
 *   kv_bit 6 (FP6-E2M3, one scale per (token, head) row of 64 - fp6_quant_e2m3_per_token_cuda on head_dim 64, group 64):
 *     codes  uint8 [2 (K, V), batch, max_len, heads, 48]: the row's 64 elements as dense 6-bit OCP E2M3 codes, element j at bits
 *            6 j .. 6 j + 5 of the row's 48 bytes read as one little-endian number (fpq_quant_rows_codes_fp6's bit format);
 *     scales fp16  [2, batch, max_len, heads].
 *   kv_bit 4 (FP4-E2M1, one scale per group of 128 consecutive elements of the flattened cache - fp_quant_e2_per_group_cuda):
 *     codes  uint8 [2, batch, max_len, heads, 32]: OCP E2M1 nibbles, element 2i in the low nibble of byte i (fpq_quant_rows_codes_mx);
 *     scales fp16  [2, batch, max_len, heads / 2]: scale g covers heads 2g and 2g + 1 (heads must be even).
 * An entry decodes to (half)((float)level(code) * (float)scale) - bit for bit the fp16 value fpq_kv_cache_step leaves in the fp16
 * cache for the same row, signed zeros, all-zero rows and rows with a subnormal fp16 scale included.  The K slab is followed by
 * the V slab in both arrays; both 16-byte aligned.
 *
 * fpq_kv_pack: quantizes the fresh fp16 rows new_k / new_v [batch, n_new, heads, 64] (rows of heads * 64 halves contiguous,
 * batch / token pitch in elements, multiples of 8, free - views of a fused qkv output need no copy; 16-byte aligned) straight
 * into the code and scale slots [pos, pos + n_new) of K and V, one launch.  The quantization decisions are fpq_kv_cache_step's
 * with group 64 / FPQ_E2M3 (kv_bit 6) or group 128 / FPQ_E2M1 (kv_bit 4).  Slots outside [pos, pos + n_new) are not touched;
 * new_k / new_v must not overlap the codes or scales.  head_dim must be 64, pos + n_new <= max_len, batch <= 65535.
 *
 * fpq_attention_blhc_kvcodes: fpq_attention_blhc over lkv = n_packed + n_new keys, bit for bit: keys [0, n_packed) are the
 * decoded packed entries of slots [0, n_packed), keys [n_packed, lkv) the fp16 rows new_k / new_v [batch, n_new, heads, 64]
 * (pitches as fpq_kv_pack's; the step's own entries, which attention sees unquantized).  The decode happens between the
 * global load and the LDS write of fpq_attention_blhc's staging, so tiles, summation order and rounding are that kernel's and
 * its error bound holds unchanged.  Nothing past slot n_packed of the codes / scales and nothing outside the q / new_k / new_v
 * views is read.  q, out, head_dim, pitches and scale as in fpq_attention_blhc; new_k / new_v may be NULL when n_new == 0,
 * codes / scales when n_packed == 0.  out must not overlap any input.
 *
 * Both: every argument error (negative sizes, kv_bit not 4 or 6, odd heads with kv_bit 4, head_dim != 64, a range past
 * max_len, a pitch not a multiple of 8, NULL or unaligned pointers, lkv == 0, scale <= 0) returns FPQ_ERR_ARG before anything
 * is launched; batch == 0 (and lq == 0, n_new == 0 where the call has nothing to do) returns FPQ_OK.  Nothing is allocated,
 * the work is ordered on `stream` and can be captured in a graph. */
int fpq_kv_pack(uint8_t* codes, void* scales, int kv_bit, int64_t batch, int64_t max_len, int64_t heads, int64_t head_dim, int64_t pos,
                const void* new_k, const void* new_v, int64_t new_batch_pitch, int64_t new_token_pitch, int64_t n_new,
                fpq_stream_t stream);
int fpq_attention_blhc_kvcodes(const void* q, const uint8_t* codes, const void* scales, int kv_bit, int64_t max_len, int64_t n_packed,
                               const void* new_k, const void* new_v, int64_t new_batch_pitch, int64_t new_token_pitch, int64_t n_new,
                               void* out, int64_t batch, int64_t lq, int64_t heads, int64_t head_dim, int64_t q_batch_pitch,
                               int64_t q_token_pitch, float scale, fpq_stream_t stream);

/* The reference's pure-torch quantizers ("CPU path", also what QuantizedLinear uses on
 * the GPU for per_channel / per_token FP4, tr/quant_utils.py:699-704,796-807):
 *     fp_quant_e{1,2,3}_per_token   tr/quant_utils.py:237-247,285-295,333-343   (clamp3 = 1)
 *     fp_quant_e{1,3}_per_group     :250-262,346-358                            (clamp3 = 1)
 *     fp_quant_e2_per_group         :298-310                                    (clamp3 = 0)
 * Same scale / normalise arithmetic as fpq_quant_rows, but the lookup is
 * quantize_to_nearest_grid (:209-230) = torch.argmin over |x - grid|: a tie goes to the
 * SMALLER value, a NaN or +-Inf normalised value selects grid[0] (so an all-zero row
 * yields -0.0), and the result is float32 whatever the input dtype.  clamp3: clamp x to
 * [-3, 3] first.  The input is never written (the reference's fp_quant_e2_per_group
 * divides its argument in place; that side effect is not reproduced). */
int fpq_quant_rows_argmin(const void* x, float* out, int64_t rows, int64_t cols, int table_id, int in_dtype,
                          int clamp3, fpq_stream_t stream);

/* Asymmetric neg/pos dual format: x <= 0 is scaled and rounded on `neg_table`,
 * x > 0 on `pos_table`, each with its own per-row scale; NaN elements take
 * neither side and come out 0 (torch.where semantics).
 *     fp_quant_e1m2_neg_e2m1_pos_per_group_cuda   tr/quant_utils.py:415-452
 *     fp6_quant_int_neg_e2m3_pos_per_group_cuda   :577-611
 *     fp6_quant_int_neg_e2m3_pos_per_token_cuda   :614-646
 *     fp4_afpq_per_group_cuda (E2M1_NEG / E2M1_POS)   models_fp_quant/quant_utils.py:498-535
 * clip_absmax: NULL, or a device scalar (in_dtype) holding max|x| over the WHOLE
 * tensor as written by fpq_absmax; the kernel then clamps x to
 * +-(T)(clip_strength * absmax) first (tr/quant_utils.py:421-422).  A NaN bound
 * turns every element into NaN, hence the whole output into zeros, exactly as
 * torch.clamp does.
 * nan_flag: NULL, or 8 bytes of device scratch (8-byte aligned) that are ZERO on entry.  With
 * clip_strength == 1.0 the clamp is the identity unless x holds a NaN (then the bound is NaN and
 * the result all zeros); passing scratch here reproduces exactly that WITHOUT the absmax pass: the
 * kernel raises word 0 when it meets a NaN and a second, 64-workgroup launch (which exits at once
 * when the flag is clear) zero-fills `out` and leaves the scratch zero again - allocate and zero it
 * once, reuse it for every call on the same stream (two launches per call, no memset; a captured
 * graph replays correctly).  Calls that may overlap on different streams need their own scratch. */
int fpq_quant_rows_dual(const void* x, void* out, int64_t rows, int64_t cols, int neg_table,
                        int pos_table, int in_dtype, int out_dtype, const void* clip_absmax,
                        float clip_strength, void* nan_flag, fpq_stream_t stream);

/* `fc2.act_quant(act(y))` of the reference's FFN in ONE pass over y (tr/basic_var.py:120-121: act = GELU(approximate="tanh");
 * fc2's input quantizer is bound at tr/quant_utils.py:991 (W4A4: fp_quant_e1m2_neg_e2m1_pos_per_group_cuda) and :930-931 (W6A6:
 * fp6_quant_int_neg_e2m3_pos_per_token_cuda)): out = fpq_quant_rows_dual(half(gelu_tanh(float(y)))) on fp16 rows of `cols`
 * elements - 128 (per group) or the token's row (per token, cols % 8 == 0, <= 16384) - for any dual table pair.  nan_flag: the
 * FP4 pair's global-clamp rule at clipping strength 1.0 (as in fpq_quant_rows_dual), NULL for the FP6 pairs (the reference
 * does not clamp there).  gelu_out: NULL, or fp16 [rows, cols] receiving the GELU values the quantizer saw (the quantization is
 * bit-exact on those; they sit within one fp16 ulp of torch's GELU on every fp16 input).  The same fused tail inside the fc1
 * GEMM: fpq_gemm_fp4_gelu_dual. */
int fpq_gelu_quant_rows_dual(const void* y, void* out, void* gelu_out, int64_t rows, int64_t cols, int neg_table, int pos_table,
                             void* nan_flag, fpq_stream_t stream);

/* The pure-torch twin of the FP4 dual format, fp_quant_e1m2_neg_e2m1_pos_per_group (tr/quant_utils.py:381-412;
 * what models_fp_quant_rotate's QuantizedLinear_fc2 binds, rot/quant_utils.py:779): same split and scales as
 * fpq_quant_rows_dual, but BOTH halves of every element go through the argmin lookup (the other half's input
 * is 0), a tie takes the smaller value, a NaN / +-Inf normalised value takes table[0] (so a group without
 * negatives adds -max|neg table| to every element - the reference's behaviour, reproduced, not fixed), and
 * the result is float32: out = (q_neg + q_pos) * (x <= 0 ? s_neg : s_pos).  clip_absmax as in
 * fpq_quant_rows_dual (the reference always clamps; pass fpq_absmax's result). */
int fpq_quant_rows_dual_argmin(const void* x, float* out, int64_t rows, int64_t cols, int neg_table, int pos_table,
                               int in_dtype, const void* clip_absmax, float clip_strength, fpq_stream_t stream);

/* "Neg reverse" rows: out = (T)( (q(x_nr / s_nr) * s_nr - m) + q(x_pos / s_pos) * s_pos ) with
 * m = |min(row)|, x_nr = (T)(min(x, 0) + m), both scales (T)(absmax / max|table|); products,
 * the subtraction and the sum in fp32.  `dtype` is the type of both x and out.
 *   replaces fp_neg_reverse_quant_per_group_cuda   models_fp_quant/quant_utils.py:454-495
 *   (the reference uses FPQ_E2M1 and cols = 128; any symmetric table and row length work).
 * A NaN in a row makes m NaN, hence the whole row NaN, as torch.min does. */
int fpq_quant_rows_neg_reverse(const void* x, void* out, int64_t rows, int64_t cols, int table_id,
                               int dtype, fpq_stream_t stream);

/* Online rotate fused in front of the per-group(128) quantizer.
 * Replaces, for the block-diagonal randomized-Hadamard rotation
 * (rotate_utils/rotation_utils.py:69-104: every 128x128 block = diag(D).H128/sqrt(128)),
 *     x1 = torch.matmul(producer.mul(s), Q)            tr/basic_var.py:263,266 (fp16 autocast)
 *     q  = fp_quant_e{1,2,3}_per_group_cuda(x1, 4, 128) / fp6_quant_*_per_group_cuda
 * by one launch:  h = half(x * s);  y = half(c_h * FWHT128(h * D));  out = quant(y).
 * x: [rows, cols] F16 or F32 (the producer's output), cols % 128 == 0;
 * smooth: device float[cols] (the GALT factor s of this block) or NULL;
 * sign_mask_host: HOST pointer to 4 x uint32, bit j set <=> D[j] == -1 (seed-42 vector);
 * out: fp16 [rows, cols]; rotated_out: NULL, or fp16 [rows, cols] receiving y.
 * Parity: out == fpq_quant_rows(y) bit for bit; y = half(c_h * sum) with the +-h_j summed in fp32 (on the matrix
 * cores; exact for groups of like magnitude): |y - exact| <= 1/2 fp16 ulp + 2^-22 c_h sum|h_j|, i.e. within 1 fp16
 * ulp of the fp64-accumulated half(x*s) @ half(Q) except on cancelling outputs of groups spanning > 2^13 in magnitude
 * (the reference GEMM's summation order is unspecified, and its +-c_h operands round more).  A non-finite input
 * poisons its own group of 128 only (the reference's dense GEMM with the block-diagonal Q: its whole row, 0 * inf).
 * x may be F32: the kernel then reads 16 bytes per lane all the same.  All pointers 16-byte aligned. */
int fpq_rotate_quant_rows(const void* x, void* out, void* rotated_out, int64_t rows, int64_t cols,
                          int in_dtype, const float* smooth, const uint32_t* sign_mask_host, int table_id,
                          fpq_stream_t stream);

/* The complete producer of tr/basic_var.py:263 / :266 plus the activation quantizer, one launch:
 *     h   = half( ((LayerNorm(x) * half(scale + 1)) + shift) * smooth )    (no affine, eps; fp32 ops in
 *                                                                            the reference's order)
 *     y   = half( c_h * FWHT128(h * D) )          (= h @ half(Q_block))
 *     out = per-group(128) quant(y)
 * x: [rows, cols] F16/F32 (F32 is what the reference's autocast run carries: tr/var.py:209, tr/basic_var.py:264,267),
 * cols % 128 == 0, cols <= 4096; scale, shift: [rows / rows_per_batch, cols]
 * in mod_dtype (the block's AdaLN scale1/shift1 or scale2/shift2, one row per batch element);
 * smooth: device float[cols] or NULL; sign_mask_host as in fpq_rotate_quant_rows.
 * h_out / rotated_out: NULL or fp16 [rows, cols] receiving h / y (for verification).
 * Parity: out == fpq_quant_rows(y) bit for bit and y as in fpq_rotate_quant_rows given h; h itself
 * matches torch's chain up to the fp32 rounding of LayerNorm's mean / rstd (1 fp16 ulp on rare
 * elements) - torch's Welford reduction order is not a contract. */
int fpq_adaln_rotate_quant_rows(const void* x, void* out, void* h_out, void* rotated_out, int64_t rows,
                                int64_t cols, int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                int64_t rows_per_batch, float eps, const float* smooth,
                                const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);

/* The same producer for the per-token configurations (W6A6, run.sh:7 with --rotate --block_rotate): the quantizer
 * behind the rotation is fp6_quant_{e2m3,e3m2}_per_token_cuda (tr/quant_utils.py:503-534), ONE scale per token row
 * of `cols` channels.  A row lives in one wavefront: cols <= 2560 (d30: 1920, d36: 2304).  row_scales: NULL or fp16
 * [rows] receiving the scales.  Parity as fpq_adaln_rotate_quant_rows: out == fpq_quant_rows(y, cols = row length)
 * bit for bit on the rotated y produced here.  The _codes_fp8 form emits the operand format of fpq_gemm_fp8_rows
 * (E4M3 bytes [rows, cols] + fp16 row scales) instead of values. */
int fpq_adaln_rotate_quant_token_rows(const void* x, void* out, void* h_out, void* rotated_out, void* row_scales,
                                      int64_t rows, int64_t cols, int in_dtype, const void* scale, const void* shift,
                                      int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                                      const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);
int fpq_adaln_rotate_quant_token_rows_codes_fp8(const void* x, uint8_t* codes, void* row_scales, int64_t rows,
                                                int64_t cols, int in_dtype, const void* scale, const void* shift,
                                                int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                                                const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);
/* ... and the _codes_fp6 form the operand format of fpq_gemm_fp6_rows (dense 6-bit E2M3 codes [rows, cols * 3 / 4] +
 * fp16 row scales): table_id must be FPQ_E2M3, cols % 32 == 0, codes 8-byte aligned. */
int fpq_adaln_rotate_quant_token_rows_codes_fp6(const void* x, uint8_t* codes, void* row_scales, int64_t rows,
                                                int64_t cols, int in_dtype, const void* scale, const void* shift,
                                                int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                                                const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);

/* max|x| over n elements (NaN-propagating, like torch's x.abs().max()), written
 * as ONE scalar of `dtype` to `out`.  `out` must hold 4 bytes; it is zeroed on the
 * stream first (hipMemsetAsync) and then combined with device atomics. */
int fpq_absmax(const void* x, int64_t n, int dtype, void* out, fpq_stream_t stream);

/* Many tensors, ONE launch (weight calibration: every Linear a rank owns, QuantizedLinear.from_float's
 * fp_quant_e{1,2,3}_per_group_cuda / fp6_quant_*_per_group_cuda on the fp32 weight, tr/quant_utils.py:828-855,
 * with the driver's later var.half() as the F16 output form).  Same results as fpq_quant_rows per segment.
 * segments_device: DEVICE-resident array of n_segments descriptors (the caller uploads it once and reuses it);
 * every segment is `rows` contiguous rows of `cols` elements, x and out 16-byte aligned; segments may have
 * different row counts, max_rows = the largest (sizes the grid: grid.y = segment, workgroups beyond a shorter
 * segment's end exit at once).  This version: cols == 128, in_dtype F32, out_dtype F16 or F32, n_segments <= 65535.
 * The descriptors' pointers are NOT validated (they live on the device): the caller guarantees them. */
typedef struct {
  const void* x;
  void* out;
  int64_t rows;
} fpq_segment_t;
int fpq_quant_rows_segments(const fpq_segment_t* segments_device, int n_segments, int64_t max_rows, int64_t cols,
                            int table_id, int in_dtype, int out_dtype, fpq_stream_t stream);

/* A few tensors, one call: the reference quantizes independent tensors back to back in places - the cached K and
 * the cached V of a generation step (tr/basic_var.py:192-200: two fp6_quant_e2m3_per_token_cuda / two
 * fp_quant_e2_per_group_cuda calls), the samples of a format search.  segments_host: HOST array (read before the
 * call returns; the descriptors travel in the kernel arguments, nothing is copied to the device), every segment
 * `rows` contiguous rows of `cols` elements; same results as fpq_quant_rows per segment.  ONE launch when
 * in_dtype == out_dtype == F16, n_segments <= 8, cols in {8, 16, ..., 512} and everything 16-byte aligned; otherwise
 * one launch per segment behind the same call. */
int fpq_quant_rows_multi(const fpq_segment_t* segments_host, int n_segments, int64_t cols, int table_id, int in_dtype,
                         int out_dtype, fpq_stream_t stream);

/* Per-tensor quantizer of the reference's pure-torch path (BASELINE.json config 1):
 *   replaces fp_quant_e2_per_tensor   search/baseline/plot_weight_distribution_for_motivation.py:285-294
 *     scale = x.abs().max() / max|table|     (two 0-dim tensors: float32 for F16 and F32 input alike)
 *     out   = table[argmin_j |T(x / scale) - table[j]|] * scale      (float32; T = x's dtype)
 * with torch.argmin's rules (first minimal index = the smaller value on a tie, NaN / +-Inf -> table[0]).
 * x: n elements F16 or F32; out: float32 [n]; scale_out: ONE float32 (the function's second result);
 * workspace: FPQ_TENSOR_WORKSPACE_BYTES of device scratch (per-workgroup maxima; no memset, no atomics).
 * Two launches (maxima, then the elementwise pass).  n == 0 stores scale 0. */
#define FPQ_TENSOR_WORKSPACE_BYTES 8192
int fpq_quant_tensor_argmin(const void* x, float* out, float* scale_out, void* workspace, int64_t n, int table_id,
                            int in_dtype, fpq_stream_t stream);

/* The loss of the per-layer format search (search/search_fp6_format.py:589-608 and its FP4 twin: per sample
 * mean((x_j W^T - q_a(x_j) q_w(W)^T)^2), summed over the samples) for up to four candidates against one reference:
 *   out[p] = sum_r row_weight[r] * sum_c (f32(ref[r, c]) - f32(y[p][r, c]))^2          p < planes
 * ref: [rows, cols]; y: [planes, rows, cols] contiguous; both `dtype` (FPQ_F16 or FPQ_F32); row_weight: [rows] float32,
 * FINITE AND POSITIVE (1 / (rows_j * cols) of the row's sample); out: `planes` float32, overwritten, not accumulated;
 * 1 <= planes <= 4.  A workgroup reads its part of ref once and every plane against it: 1 + planes matrices move.
 * The subtraction, the square and every sum are fp32; nothing is rounded to fp16.
 * workspace: FPQ_SQERR_WORKSPACE_BYTES of device scratch (one partial per plane and workgroup, the grid is capped at
 * FPQ_SQERR_WORKSPACE_BYTES / 16 workgroups).  No memset, no atomics: the same inputs give the same bits on every call
 * whatever the workspace held.  Two launches (partials, then one workgroup sums them in a fixed order); no host
 * synchronisation, allocation or copy - legal inside a stream capture.
 * Checked before anything is enqueued, in this order:
 *   a NULL pointer, rows < 0, cols < 0, planes outside 1 .. 4                                     FPQ_ERR_ARG
 *   dtype other than FPQ_F16 / FPQ_F32                                                           FPQ_ERR_DTYPE
 *   cols == 0, cols % 8 != 0 (F16) or cols % 4 != 0 (F32), rows > 2^31 - 1
 *     (or planes x rows x cols beyond 63 bits)                                                   FPQ_ERR_SHAPE
 *   ref, y or row_weight not 16-byte aligned (out, workspace: 4-byte)                             FPQ_ERR_ARG
 * rows == 0 stores `planes` zeros (one launch) and succeeds.
 * Accuracy: every term is non-negative and every weight positive, so against the exact sum S of the stored inputs
 *   |out[p] - S| <= (D + c) 2^-24 S,    D = V + n_it + 26,  c = 3
 * V = 8 (F16) / 4 (F32) additions inside a 16-byte vector, n_it = ceil(n_vec / (min(ceil(n_vec / 256), 2048) * 256))
 * additions in a lane (n_vec = rows cols / V), 6 + 3 in the workgroup, 8 + 6 + 3 over the partials; c = the roundings of the
 * difference, the square and the weight.  [13600 x 5760] F16: n_it = 19, (D + c) 2^-24 = 3.4e-6.  F32 inputs whose squares or
 * weighted squares go subnormal add at most 2^-149 per element and per vector (F16 inputs cannot: the smallest non-zero
 * difference squared is 2^-48).
 * Non-finite inputs behave as the fp32 expression does: out[p] is NaN if any difference of plane p is NaN (a NaN input, or
 * inf - inf), otherwise +inf if any difference (or an fp32 square) is infinite; the other planes are not touched by it. */
#define FPQ_SQERR_WORKSPACE_BYTES 32768
int fpq_sqerr_rows_weighted(const void* ref, const void* y, const float* row_weight, float* out, void* workspace,
                            int64_t rows, int64_t cols, int planes, int dtype, fpq_stream_t stream);

/* Codeword output (build-defined; the reference's kernel never emits codes,
 * quant_kernel.cu:18,49).  code = index into the sorted, de-duplicated table
 * (0..14 for the FP4 tables, 0..62 for FP6); for the FP4 tables two codes are
 * packed per byte (element 2i in the low nibble).  scales: one per row, in
 * x's dtype.  dequant: table_dedup[code] * scale reproduces fpq_quant_rows. */
int fpq_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols,
                         int table_id, int in_dtype, int pack_nibbles, fpq_stream_t stream);

/* ---- F2: a real FP4 consumer --------------------------------------------
 * Per-group(128) FP4-E2M1 quantization straight to HARDWARE codes: one OCP E2M1 nibble per element
 * (bit 3 sign, bits 2:0 index into {0,.5,1,1.5,2,3,4,6}; element 2i in the low nibble of byte i) and
 * one scale per group in x's dtype.  Same scale / normalise / rounding arithmetic as fpq_quant_rows,
 * i.e. level * scale reproduces fp_quant_e2_per_group_cuda exactly.  x: [rows, cols] F16 or F32,
 * cols % 128 == 0; codes: [rows, cols/2]; scales: [rows, cols/128]. */
int fpq_quant_rows_codes_mx(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols,
                            int in_dtype, fpq_stream_t stream);

/* The fused producers of F1 emitting the FP4 GEMM's operand format directly (hardware E2M1 codes + one fp16
 * scale per 128-group) instead of fake-quantized values: same arguments and the same arithmetic as
 * fpq_rotate_quant_rows / fpq_adaln_rotate_quant_rows with table FPQ_E2M1, i.e. level(code) * scale is bit-equal
 * to their `out`.  codes: [rows, cols/2]; scales: fp16 [rows, cols/128].  With these the activation never exists
 * in HBM as fp16 between the block's LayerNorm and its matrix product (2 B read + 0.53 B written per element). */
int fpq_rotate_quant_rows_codes_mx(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols,
                                   int in_dtype, const float* smooth, const uint32_t* sign_mask_host,
                                   fpq_stream_t stream);
int fpq_adaln_rotate_quant_rows_codes_mx(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols,
                                         int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                         int64_t rows_per_batch, float eps, const float* smooth,
                                         const uint32_t* sign_mask_host, fpq_stream_t stream);

/* out[t, o] = bias[o] + sum_g a_scale[t,g] * w_scale[o,g] * dot_128(levels(a)[t,g,:], levels(w)[o,g,:])
 * on the gfx950 block-scaled FP4 matrix cores (one 16x16x128 MFMA per group and 16x16 output tile,
 * exact products, fp32 accumulation); replaces F.linear(act_quant(x), W_q, b) of
 * tr/quant_utils.py:765-767 for the W4A4 per-group E2M1 configuration.  a_codes [tokens, k/2],
 * a_scales fp16 [tokens, k/128], w_codes [outs, k/2], w_scales [outs, k/128] in w_scale_dtype,
 * bias fp16 [outs] or NULL, out fp16 [tokens, outs]; k % 128 == 0, outs % 8 == 0.
 * Numerics: does NOT round the de-quantized operands to fp16 first as the reference's fp16 GEMM does.  Against the
 * float64 product of the decoded operands every element is within
 *     2^-11 |ref| + 2^-25 + (1 + 2^-10) 2^-24 (S + R + |ref|),   S = sum_g |sa sw d_g|,  R = sum_g |exact partial sum after g|
 * (tests/gemm_model.py derives it), assuming the 128-term dot d_g of E2M1 levels is exact (multiples of 1/4, |d_g| <= 4608).
 * Per group the LDS-DMA tilings round t = d_g sa and acc = fma(t, sw, acc), the register-staged ones p = sa sw and
 * acc = fma(d_g, p, acc); out = fp16(acc + bias), nearest-even, overflow to inf, NaN / inf scales propagate as in IEEE
 * arithmetic.  Each tiling is bit-equal to an fp32 model of exactly those steps. */
int fpq_gemm_fp4_mx(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                    int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                    fpq_stream_t stream);

/* ---- F2 for the per-token / per-channel configurations (W6A6, run.sh:7) ----------------------------------------
 * Per-row quantization straight to one OCP FP8 E4M3 byte per element (every level of the symmetric FP4 / FP6 tables
 * is exactly an E4M3 number) + one scale per row in x's dtype: same arithmetic as fpq_quant_rows with cols = row
 * length, i.e. e4m3(code) * scale reproduces fp6_quant_{e2m3,e3m2}_per_token_cuda (tr/quant_utils.py:503-534) and the
 * per-channel weight quantization of QuantizedLinear.from_float (:808-829).  codes: [rows, cols]; scales: [rows]. */
int fpq_quant_rows_codes_fp8(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id,
                             int in_dtype, fpq_stream_t stream);

/* out[t, o] = bias[o] + a_scale[t] * w_scale[o] * sum_k e4m3(a[t,k]) * e4m3(w[o,k]) on the FP8 matrix cores (exact
 * products, fp32 accumulation, nothing but matrix instructions in the K loop: with one scale per row the scales
 * leave the sum); replaces F.linear(act_quant(x), W_q, b) of tr/quant_utils.py:765-767 for per_token activations x
 * per_channel weights.  a_codes [tokens, k], w_codes [outs, k], bias fp16 [outs] or NULL, out fp16 [tokens, outs];
 * k % 128 == 0, outs % 8 == 0, code arrays and out 16-byte aligned.  Numerics (and fpq_gemm_fp6_rows'): acc is chained
 * through the k / 128 MFMAs, then out = fp16(fl(fl(acc * fl(sr * sc)) + bias)).  Against the float64 product of the decoded
 * operands every element is within
 *     2^-11 |ref| + 2^-25 + (1 + 2^-10) (2^-23 R + 2^-24 (2 S + |ref|)),
 *     S = |sr sc| sum_k |La Lw|,  R = |sr sc| sum_steps (|exact partial sum before the step| + the step's sum_k |La Lw|)
 * (tests/gemm_model.py).  The rounding of the chained MFMA accumulator is not documented: the bound allows one fp32 ulp
 * per step, sound for nearest and for truncation, plus 128 * 2^-23 of each step's largest product.  Measured on an MI355X: with
 * E2M3 codes (what the W6A6 path feeds both kernels) every output is inside the bound and equals a model with one rounding
 * per step; E2M3 partial sums are exact below 2^18 (K >= 4661 with near-extreme codes of one sign to leave
 * that range).  With E3M2 or full-range E4M3 codes the matrix core's 128-term dot loses more than that (up to 5.3 times the
 * bound, already at k = 128): the bound does not hold for those codes (tests/test_gpu_gemm.py holds them to 8 times it). */
int fpq_gemm_fp8_rows(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                      const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs,
                      int64_t k, fpq_stream_t stream);

/* The same pair with the operands in the matrix instruction's 6-bit packed form (FP6 E2M3: sign, 2 exponent bits with
 * bias 1, 3 mantissa bits; element j of a row in bits [6j, 6j+6) of the row's little-endian bit string, i.e. dense
 * packing, 3/4 byte per element): 25 % less operand traffic in a kernel bound by exactly that.  table_id must be
 * FPQ_E2M3 (BF6 E3M2 - sign, 3 exponent bits with bias 3, 2 mantissa bits, same packing - through fpq_quant_rows_codes_f6 /
 * fpq_gemm_f6_rows below), cols % 32 == 0 (GEMM: k % 128 == 0); codes: [rows, cols * 3 / 4]; everything else as the FP8 pair. */
int fpq_quant_rows_codes_fp6(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id,
                             int in_dtype, fpq_stream_t stream);
int fpq_gemm_fp6_rows(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                      const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs,
                      int64_t k, fpq_stream_t stream);

/* The three GEMMs with an optional fused tail, for the AdaLN blocks' `x = x + attn(...).mul_(gamma1)` /
 * `x + ffn(...).mul(gamma2)` (tr/basic_var.py:264,267): out = residual + y * gate[t / rows_per_gate, :], y being the
 * fp16 result of the plain call, each operation in fp16 with one rounding (bit-identical to the two torch ops on y).
 * Either pointer may be NULL; `residual` may be `out` itself; both 16-byte aligned.  epilogue == NULL: the plain call. */
typedef struct fpq_gemm_epilogue {
  const void* gate;      /* fp16 [ceil(tokens / rows_per_gate), outs] or NULL (gamma viewed as [B, C]) */
  const void* residual;  /* fp16 [tokens, outs] or NULL */
  int64_t rows_per_gate; /* consecutive token rows sharing a gate row (tokens per batch entry), >= 1 */
} fpq_gemm_epilogue_t;
/* The same tail as a call of its own, for a Linear that runs elsewhere (fc2's fp16 GEMM): out = residual +
 * y * gate[row / rows_per_gate, :], all fp16 [rows, cols] (gate [ceil(rows / rows_per_gate), cols]), cols % 8 == 0,
 * 16-byte aligned; out may be y or residual. */
int fpq_gate_residual(const void* y, const void* gate, const void* residual, void* out, int64_t rows, int64_t cols,
                      int64_t rows_per_gate, fpq_stream_t stream);
int fpq_gemm_fp4_mx_ex(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                       int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                       const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
/* fc1 of the AdaLN block's FFN with everything up to fc2's GEMM in its epilogue (tr/basic_var.py:120-121; fc2's input
 * quantizer is bound at tr/quant_utils.py:991 and defined at :415-452):
 *     y   = half(dequant(a) @ dequant(w).T + bias)                         the Linear output of fpq_gemm_fp4_mx, bit for bit
 *     h   = half(gelu_tanh(float(y)))                                      F.gelu(y, approximate="tanh") on the fp16 tensor
 *     out = fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(h, 4, 128)           groups of 128 consecutive outputs, strength 1.0
 * out: fp16 [tokens, outs], outs % 128 == 0.  gelu_out: NULL, or fp16 [tokens, outs] receiving h.  nan_flag: as in
 * fpq_quant_rows_dual (8 bytes of zeroed persistent scratch: "a NaN anywhere in h => the whole result is zero", one tiny
 * second launch; NULL skips the rule).  Parity: out == fpq_quant_rows_dual(h) bit for bit on the h produced here; h within
 * one fp16 ulp of torch's GELU of y on every fp16 input (torch's formula in torch's operation order, the device library's
 * tanh restated).  Replaces three launches and 10 B of HBM traffic per element behind the GEMM. */
int fpq_gemm_fp4_gelu_dual(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                           int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                           int64_t k, void* nan_flag, fpq_stream_t stream);
int fpq_gemm_fp8_rows_ex(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                         const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                         int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
int fpq_gemm_fp6_rows_ex(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                         const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                         int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);

/* ---- K-MAJOR OPERAND IMAGES ------------------------------------------------------------------------------------------
 * The FP4 and FP6 matrix-core GEMMs above read ROW-MAJOR code tensors [rows, k/2] / [rows, k*3/4]; per K step of 128
 * elements their LDS-DMA engine then gathers 64 / 96 bytes out of each of 384 rows that lie a whole row apart, and issuing
 * those gathers is what bounds them (profiles/r05_gemm6_stamps.txt, r05_lds_dma_issue.txt: 100 - 150 cycles per 1 KiB
 * piece against 65 - 70 for a contiguous one).  The *_km entry points take the same codes as a K-MAJOR IMAGE instead:
 *
 *     image[(s * image_rows + j) * seg + p * 16 + b]      s = K step (k / 128 of them), j = image row, seg = 64 (FP4) or
 *                                                          96 (FP6) bytes, p = 16-byte chunk inside the segment, b = byte
 *   = codes[row(j), s * seg + c(j, p) * 16 + b]
 *
 *   chunk order (the GEMM's bank-conflict-free LDS image, so that a DMA piece is one linear 1 KiB copy):
 *     FP4: c = p ^ pi(j & 15),  pi(q) = (0, 2, 3, 1)[q >> 2]          FP6: c = (p - ((j >> 3) & 1)) mod 6
 *   activation side: image_rows = rows, row(j) = j (no padding: the image has exactly the row-major tensor's size);
 *   weight side ("dealt", the order the kernels hand a wavefront's 64 outputs to its four 16-row tiles):
 *     image_rows = rows rounded up to 64, row(j) = (j & ~63) + 4 * (j & 15) + ((j >> 4) & 3), zero where row(j) >= rows.
 *
 * The per-group scales of the FP4 GEMM travel the same way - row-major [rows, k/128] costs every tile 90 strided loads and as
 * many LDS writes, 8 % of the kernel - as a K-MAJOR SCALE IMAGE, always fp32:
 *     scale_image[g * image_rows + r] = (float)scales[r, g]        image_rows = rows rounded up to 4 (activation side) or to 64
 *                                                                   (weight side; natural row order, NOT dealt), padding = 0
 * (fp16 -> fp32 is exact: the GEMM multiplies the same numbers).  The FP6 GEMM's one scale per row stays a plain vector.
 *
 * Same arithmetic, same results bit for bit (tests/test_gpu_kmajor.py); bias, out and the epilogue are unchanged.
 * fpq_codes_to_kmajor / fpq_scales_to_kmajor convert row-major codes / scales (weights once at load time; any producer's
 * output as a fallback); the *_km producers below write the activation images directly.  code_bits: 4 or 6;
 * scale_dtype: FPQ_F16 or FPQ_F32; all image pointers 16-byte aligned. */
int fpq_codes_to_kmajor(const uint8_t* codes, uint8_t* image, int64_t rows, int64_t k, int code_bits, int dealt,
                        fpq_stream_t stream);
int fpq_scales_to_kmajor(const void* scales, int scale_dtype, float* image, int64_t rows, int64_t groups, int weight_side,
                         fpq_stream_t stream);
/* fpq_gemm_fp4_mx_ex / fpq_gemm_fp4_gelu_dual / fpq_gemm_fp6_rows_ex on k-major images (a_image: activation side,
 * w_image: dealt weight side).  FP4: a_scales / w_scales are k-major SCALE images (fp32: w_scale_dtype must be FPQ_F32;
 * tokens, outs < 2^28); FP6: the row scale vectors as before.  bias must be 8-byte aligned; k limited by the LDS-DMA
 * kernels' scale tiles (FP4: the row-major entry point falls back to a register-staged kernel for very long k, this one
 * returns FPQ_ERR_SHAPE). */
int fpq_gemm_fp4_mx_km(const uint8_t* a_image, const void* a_scales, const uint8_t* w_image, const void* w_scales,
                       int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                       const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
int fpq_gemm_fp4_gelu_dual_km(const uint8_t* a_image, const void* a_scales, const uint8_t* w_image, const void* w_scales,
                              int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                              int64_t k, void* nan_flag, fpq_stream_t stream);
/* WHICH TILING AN FP4 GEMM CALL RUNS.  The FP4 LDS-DMA kernels come in four tilings, named by the values of the switch
 * FPQ_GEMM_CFG that force them: 10 / 20 / 30 = 256 x 128, 128 x 128, 64 x 128 tiles behind a two-stage ring, 40 = the 64 x 128 tile
 * behind a deep ring of stage buffers whose loads span the loop's barrier (for the first scale steps, where a tile's time is its
 * chain of trips to memory).  All four share the per-group arithmetic and give the same bits.  (FPQ_GEMM_CFG 0..2 name the
 * register-staged kernel's tilings, which only a row-major one-tensor call honours; the A6W4 entry points have 20 and 30 and
 * treat every other value as "not set".)
 * fpq_gemm_fp4_tiling: the code - 10, 20, 30 or 40 - of the LDS-DMA tiling that a call of fpq_gemm_fp4_mx / _ex / _km / _split /
 * _split_qknorm (form 0) or of fpq_gemm_fp4_gelu_dual / _km (form 1: the LDS image carries the dual quantizer's bucket table too)
 * with these sizes and an 8-byte aligned bias runs under the current value of the switch, the fall-through to a smaller image where
 * the chosen one exceeds a CU's 160 KiB of LDS included.  Host arithmetic only: no GPU call, nothing launched.  Shapes the entry
 * points refuse give their code: negative sizes or another form FPQ_ERR_ARG; k % 128, k > 8192, outs % 8 (form 1: outs % 128),
 * tokens or outs above 2^31 - 1 FPQ_ERR_SHAPE; tokens == 0 or outs == 0 FPQ_OK (nothing would be launched); k == 0 FPQ_ERR_ARG. */
int fpq_gemm_fp4_tiling(int64_t tokens, int64_t outs, int64_t k, int form);
/* The activation producers writing the k-major images directly (same arguments as the forms without _km; image:
 * rows * cols / 2 bytes (FP4) or rows * cols * 3 / 4 (FP6), below 2 GiB, 16-byte aligned; cols % 128 == 0).  The FP4
 * producers' `scales` is the fp32 k-major scale image [cols / 128][rows rounded up to 4] (padding rows are not written);
 * the FP6 producers' `scales` / `row_scales` stay one value per row.
 * fpq_quant_rows_codes_mx_km: fp16 rows only.  The fused adaLN / rotation producers: the matrix-core forms only (rows of up
 * to 2560 channels for adaLN), FPQ_ERR_SHAPE otherwise - use the row-major producer + fpq_codes_to_kmajor there. */
int fpq_quant_rows_codes_mx_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int in_dtype,
                               fpq_stream_t stream);
int fpq_rotate_quant_rows_codes_mx_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                      const float* smooth, const uint32_t* sign_mask_host, fpq_stream_t stream);
int fpq_adaln_rotate_quant_rows_codes_mx_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols,
                                            int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                            int64_t rows_per_batch, float eps, const float* smooth,
                                            const uint32_t* sign_mask_host, fpq_stream_t stream);
int fpq_quant_rows_codes_fp6_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int table_id,
                                int in_dtype, fpq_stream_t stream);
int fpq_adaln_rotate_quant_token_rows_codes_fp6_km(const void* x, uint8_t* image, void* row_scales, int64_t rows, int64_t cols,
                                                   int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                                   int64_t rows_per_batch, float eps, const float* smooth,
                                                   const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);
/* The FP4 GEMM with a SPLIT OUTPUT: the outs columns are n_parts (<= 3) parts of part_cols (% 128 == 0) each, and every part has
 * its own destination: token t = b * rows_per_batch + l of part p is written to row  b * batch_stride[p] + row0[p] + l  of out[p]
 * (fp16, row_stride[p] elements per row, >= part_cols, % 4 == 0, 8-byte aligned).  What it is for: mat_qkv of an attention block
 * (tr/basic_var.py:173-209) - q to its own [B, L, H * c] tensor, k and v straight into the KV cache's slots [B, max_len, H * c] at
 * token position `len` (batch_stride = max_len, row0 = len), so that the cache's copy-in pass (60 % of the bytes
 * fpq_kv_cache_step moves) never runs: fpq_kv_cache_step then only quantizes the previous step's entries (n = 0).
 * Same arithmetic as fpq_gemm_fp4_mx_ex / _km (kmajor: 0 row-major operands, 1 k-major images); no gate / residual tail. */
typedef struct fpq_gemm_split {
  int64_t part_cols;
  int32_t n_parts;
  void* out[3];
  int64_t row_stride[3];
  int64_t rows_per_batch;
  int64_t batch_stride[3];
  int64_t row0[3];
} fpq_gemm_split_t;
int fpq_gemm_fp4_mx_split(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales, int w_scale_dtype,
                          const void* bias, int64_t tokens, int64_t outs, int64_t k, const fpq_gemm_split_t* split, int kmajor,
                          fpq_stream_t stream);
int fpq_gemm_fp6_rows_km(const uint8_t* a_image, const void* a_scales, int a_scale_dtype, const uint8_t* w_image,
                         const void* w_scales, int w_scale_dtype, const void* bias, void* out, int64_t tokens,
                         int64_t outs, int64_t k, const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);

/* THE Q / K L2 NORM of an attention block with attn_l2_norm=True (the default of every released VAR model; tr/basic_var.py:160-183):
 *     qkv = mat_qkv(x) + cat(q_bias, 0, v_bias);  q = F.normalize(q, dim=-1) * exp(min(scale_mul_1H11, log 100));  k = F.normalize(k, dim=-1)
 * before k enters the KV cache (quant(k / |k|) != quant(k) / |k|: the norm cannot follow the cache's quantization).  Under
 * autocast(float16) the Linear's output is fp16 and the fp32 bias promotes it, so with y16 the fp16 Linear output, b32 the fp32 bias
 * [3C] (or none) and s_h the per-head multiplier q_head_scale[h] (fp32, exp(min(scale_mul_1H11[h], log 100)), computed once by
 * the caller), per (token, head of 64 channels):
 *     y = float(y16) + b32                               (the bias AFTER the fp16 rounding)
 *     q_out = half(y_q / max(sqrt(sum y_q^2), 1e-12) * s_h)      k_cache = half(y_k / max(sqrt(sum y_k^2), 1e-12))      v_cache = half(y_v)
 * With r the same lines in exact arithmetic on y16 and b32, every finite element of q_out and k is within
 *     0.5 ulp16(|r|) (1 + 2^-12) + 16 * 2^-24 |r|            (ulp16 floored at 2^-24: subnormal results included)
 * of r - fp32 throughout (a real square root and quotient), one fp16 rounding at the end; the derivation is the docstring of
 * tests/qknorm_model.py bound(), for sum y^2 < 2^120.  v bit for bit; a zero row gives zeros.  NON-FINITE ROWS follow the
 * reference's fp32 lines element for element: a NaN anywhere in a head makes its 64 outputs NaN; a head with +-inf and no NaN
 * gets NaN at the inf elements and (signed) zeros at the others; |r| >= 65520 is +-inf.  The cache's quantization of these entries
 * at the next step is fpq_kv_cache_step's, unchanged.
 *
 * fpq_gemm_fp4_mx_split_qknorm: fpq_gemm_fp4_mx_split with that epilogue: n_parts == 3 (q, k, v), part_cols % 128 == 0, heads of 64
 * columns (part_cols / 64 of them), bias fp32 [3 * part_cols] 16-byte aligned or NULL, q_head_scale fp32 [part_cols / 64].
 * Anything else: FPQ_ERR_ARG before any launch. */
int fpq_gemm_fp4_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales,
                                 int w_scale_dtype, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                 const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream);
/* The FP6 row-scaled GEMM (fpq_gemm_fp6_rows_ex, kmajor = 0 / fpq_gemm_fp6_rows_km, kmajor = 1; operands, scale dtypes and every
 * check as there, no gate / residual tail) with the SPLIT OUTPUT of fpq_gemm_fp4_mx_split, and with the Q / K L2 NORM above in that
 * epilogue: the W6A6 mat_qkv.  Without the norm every written value is bit for bit the one fpq_gemm_fp6_rows_ex / _km writes at
 * that (token, column); with it, y16 is what they write with bias == NULL and q, k, v follow the contract above (the arithmetic of
 * fpq_gemm_fp4_mx_split_qknorm: on operands that represent the same matrices the two GEMMs write the same bits).
 * split: n_parts 1..3 (exactly 3 with the norm), part_cols % 128 == 0, outs == n_parts * part_cols, rows_per_batch >= 1 and
 * tokens % rows_per_batch == 0; EVERY destination out[p] non-NULL and 8-byte aligned, row_stride[p] >= part_cols and % 4 == 0,
 * batch_stride[p], row0[p] >= 0.  bias: fp16 [outs] or NULL (split); fp32 [3 * part_cols], 16-byte aligned, or NULL (norm);
 * q_head_scale fp32 [part_cols / 64], never NULL.  Anything else: FPQ_ERR_ARG (FPQ_ERR_SHAPE / FPQ_ERR_DTYPE as fpq_gemm_fp6_rows_ex
 * uses them) before any launch; tokens == 0: FPQ_OK, nothing launched. */
int fpq_gemm_fp6_rows_split(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes, const void* w_scales,
                            int w_scale_dtype, const void* bias, int64_t tokens, int64_t outs, int64_t k, const fpq_gemm_split_t* split,
                            int kmajor, fpq_stream_t stream);
int fpq_gemm_fp6_rows_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, const uint8_t* w_codes,
                                   const void* w_scales, int w_scale_dtype, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                   const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream);
/* ---- A format per operand on the FP6 path: FP6 E2M3 or BF6 E3M2 ---------------------------------------------------------------
 * The matrix instruction decodes each operand by a selector of its own, so the 6-bit path serves all four pairs of the
 * reference's FP6 format search (E2M3 / E3M2 activations x E2M3 / E3M2 weights).  Both formats use the dense packing of
 * fpq_quant_rows_codes_fp6 (element j of a row in bits [6j, 6j+6) of the row's little-endian bit string); a code is
 *     FPQ_E2M3 (FP6): sign, 2 exponent bits (bias 1), 3 mantissa bits: 0, 1/8 .. 7/8, 1 .. 7.5
 *     FPQ_E3M2 (BF6): sign, 3 exponent bits (bias 3), 2 mantissa bits: 0, 1/16 .. 3/16, 1/4 .. 28
 * - level for level the reference's tables (tr/quant_utils.py:458-486); a zero level of either sign is code 0.  Row-major codes and
 * k-major images (fpq_codes_to_kmajor(.., 6, ..)) have the same layout for both formats: only the decoder differs.
 * table_id / a_table / w_table: FPQ_E2M3 or FPQ_E3M2; anything else is FPQ_ERR_TABLE, decided before any other check and before a
 * device is touched.  kmajor != 0: the k-major form of the entry point the call otherwise equals.  With FPQ_E2M3 (on both sides)
 * every call launches exactly what the entry point it extends launches; those keep refusing FPQ_E3M2.
 *   fpq_quant_rows_codes_f6                      = fpq_quant_rows_codes_fp6 / _fp6_km: the decisions of fpq_quant_rows(.., table_id)
 *   fpq_adaln_rotate_quant_token_rows_codes_f6   = fpq_adaln_rotate_quant_token_rows_codes_fp6 / _fp6_km
 *   fpq_gemm_f6_rows                             = fpq_gemm_fp6_rows_ex / fpq_gemm_fp6_rows_km (a: activations, w: weights)
 *   fpq_gemm_f6_rows_split, .._split_qknorm      = fpq_gemm_fp6_rows_split, fpq_gemm_fp6_rows_split_qknorm
 * Scale dtypes: (FPQ_E2M3, FPQ_E2M3) takes all four pairs as fpq_gemm_fp6_rows_ex does; a pair with an FPQ_E3M2 side takes fp16
 * ACTIVATION scales (what the activation quantizers and the adaLN producer write) with fp16 or fp32 weight scales - fp32 activation
 * scales there are FPQ_ERR_DTYPE (the kernels are not compiled: they would double the compile time of the GEMM unit).
 * Numerics: the arithmetic and the bound of fpq_gemm_fp8_rows (above).  As stated there, the matrix core's 128-term dot of E3M2
 * levels loses more than the derived bound allows - measured through the FP8 GEMM: up to 5.3 times - and the project holds those
 * levels to 8 times the bound (tests/gemm_model.py, WIDE_FP8_MEASURED).  The same levels in the 6-bit operand form get the same
 * allowance wherever a side holds E3M2 levels (tests/test_gpu_bf6.py); (FPQ_E2M3, FPQ_E2M3) stays within 1.0 times the bound.
 * Measured on an MI355X in the BF6 form (profiles/r08_bf6_gemm_bound.txt): at most 1.85 times the bound (E3M2 x E3M2 with a bias that
 * cancels the product), below 1.0 for every mixed pair; bit-equal to fpq_gemm_fp8_rows on the same levels as E4M3 bytes in all but a few
 * elements - the 6-bit and the 8-bit operand form of a level are rounded alike. */
int fpq_quant_rows_codes_f6(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                            int kmajor, fpq_stream_t stream);
int fpq_adaln_rotate_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols,
                                               int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                               int64_t rows_per_batch, float eps, const float* smooth,
                                               const uint32_t* sign_mask_host, int table_id, int kmajor, fpq_stream_t stream);
int fpq_gemm_f6_rows(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                     const void* w_scales, int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs,
                     int64_t k, const fpq_gemm_epilogue_t* epilogue, int kmajor, fpq_stream_t stream);
int fpq_gemm_f6_rows_split(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                           const void* w_scales, int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                           const fpq_gemm_split_t* split, int kmajor, fpq_stream_t stream);
int fpq_gemm_f6_rows_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                                  const void* w_scales, int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs,
                                  int64_t k, const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream);

/* ---- A6W4: E1M2 / E3M0 activations x E2M1 weights, per group of 128 ------------------------------------------------------
 * The reference's mixed W4A4 model (quantize_VAR_mixed_fp4_datatype / quantize_VAR_use_different_datatype) gives fc1 and mat_qkv
 * an E3M0 or E1M2 ACTIVATION format in most blocks and keeps every weight E2M1.  The matrix instruction decodes only E2M1 from
 * nibbles, but it takes a format selector per operand and runs 6-bit operands at the FP4 rate; every E1M2 level (0, 0.25 ..
 * 1.75) is an FP6 E2M3 number and every E3M0 level (0, 0.25, 0.5, 1 .. 16) a BF6 E3M2 number.
 *
 * fpq_quant_rows_codes_g6: per-group(128) quantization on table_id = FPQ_E1M2 or FPQ_E3M0 (anything else: FPQ_ERR_TABLE) straight
 * to dense 6-bit hardware codes - the E2M3 codes of E1M2 levels, the E3M2 codes of E3M0 levels, in the bit format of
 * fpq_quant_rows_codes_fp6 (element j of a row in bits [6j, 6j + 6) of the row's little-endian bit string) - and one scale per
 * group in x's dtype.  x: [rows, cols] F16 or F32, cols % 128 == 0; codes: [rows, cols * 3 / 4]; scales: [rows, cols / 128];
 * x and codes 16-byte aligned.  Same scale / normalise / rounding arithmetic as fpq_quant_rows(table_id, cols = 128): level(code)
 * * scale (one product in x's dtype) reproduces fp_quant_e1_per_group_cuda / fp_quant_e3_per_group_cuda bit for bit.  A group
 * whose maximum is not finite is handled as fpq_quant_rows_codes_mx handles it: the maximum itself (+inf, or the NaN) is stored as
 * the group's scale and every element gets the code of the level the quantizer's table lookup gives it, so level(code) * scale
 * is again what fpq_quant_rows writes (NaN from 0 * inf or anything * NaN, +-inf where a non-zero level meets an infinite scale):
 * the non-finite value travels in the SCALE, every code is a valid code.  An all-zero group has scale 0 and code 0 throughout.
 *
 * fpq_gemm_a6w4_mx: out[t, o] = fp16(bias[o] + sum_g a_scale[t,g] * w_scale[o,g] * dot_128(level(a)[t,g,:], level(w)[o,g,:])), with
 * the optional gate / residual tail of fpq_gemm_epilogue_t (NULL: none).  a_codes: 6-bit [tokens, 3 k / 4] of a_table (FPQ_E1M2:
 * decoded as FP6 E2M3, cbsz = 2; FPQ_E3M0: as BF6 E3M2, cbsz = 3; anything else FPQ_ERR_TABLE), a_scales fp16 [tokens, k / 128];
 * w_codes / w_scales / w_scale_dtype exactly what fpq_gemm_fp4_mx takes (E2M1 nibbles [outs, k / 2], blgp = 4): one stored FP4
 * weight serves both GEMMs.  Shape and alignment rules of fpq_gemm_fp4_mx_ex (k % 128 == 0, k <= 8192, outs % 8 == 0, codes and
 * out 16-byte aligned), checked before any launch; the bias must be 8-byte aligned (there is no register-staged form to fall
 * back to).  Row-major operands; k-major images: fpq_gemm_a6w4_mx_km below.  The split output and the q / k norm:
 * fpq_gemm_a6w4_mx_split / fpq_gemm_a6w4_mx_split_qknorm below; the fc1 tail: fpq_gemm_a6w4_gelu_dual.
 * Numerics: the per-group steps of fpq_gemm_fp4_mx's LDS-DMA tilings - t = fl(d_g sa), acc = fma(t, sw, acc), out = fp16(acc +
 * bias).  Products of an E3M0 or E1M2 level and an E2M1 level are multiples of 1/8 (|product| <= 96 resp. 10.5), so the exact
 * 128-term dot d_g has at most 17 significant bits (|d_g| <= 12288) and fits the fp32 accumulator.
 * MEASURED on an MI355X before anything else (profiles/r09_a6w4_dot.txt): with k = 128, unit scales and no bias, dots that are fp16
 * numbers - the largest products cancelling beside a few +-1/8, all 15 x 15 level pairs alone and 128-fold, the largest product
 * beside 127 smallest - come out bit for bit for both formats: the matrix core keeps every product (it does not for full-range
 * E3M2 x E3M2 codes, see fpq_gemm_f6_rows).  So the contract is fpq_gemm_fp4_mx's, unchanged: against the float64 product of the
 * decoded operands every element is within 2^-11 |ref| + 2^-25 + (1 + 2^-10) 2^-24 (S + R + |ref|) (allowance 1.0; worst measured
 * over the shape sweep 1.000 x the bound, the fp16 output rounding), and the output is bit-equal to an fp32 model of those steps
 * (tests/a6w4_model.py, tests/test_gpu_a6w4.py).  Both tilings (64 x 128 and 128 x 128 tiles) share the K order: bit-equal. */
int fpq_quant_rows_codes_g6(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                            fpq_stream_t stream);
int fpq_gemm_a6w4_mx(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                     int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                     const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
/* fpq_gemm_a6w4_gelu_dual: fpq_gemm_fp4_gelu_dual for a 6-bit activation - fc1 of the FFN, its GELU(tanh) and fc2's dual E1M2- /
 * E2M1+ per-group(128) input quantizer in ONE launch (+ the NaN fix-up launch): out = fp16 [tokens, outs] =
 * fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(gelu_tanh(y), 4, 128) with y the fp16 [tokens, outs] that fpq_gemm_a6w4_mx writes for
 * the same operands and bias, bit for bit.  Operands (a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, bias) exactly
 * fpq_gemm_a6w4_mx's, row-major; (k-major images: fpq_gemm_a6w4_gelu_dual_km below); the tail, gelu_out (NULL, or fp16 [tokens, outs], 16-byte aligned: the GELU values the quantizer
 * saw), nan_flag (NULL, or the 8-byte zeroed scratch of fpq_quant_rows_dual: a NaN in any live row makes the whole result +0 and
 * the scratch is zero again afterwards) exactly fpq_gemm_fp4_gelu_dual's - the same GELU of the same fp16 value and the same
 * quantizer arithmetic, so the two entry points agree bit for bit wherever their Linear outputs do.
 * Checks, in this order, before any launch: a_table (FPQ_ERR_TABLE), negative sizes (FPQ_ERR_ARG), w_scale_dtype (FPQ_ERR_DTYPE),
 * shape (FPQ_ERR_SHAPE: k % 128, k > 8192, outs % 128 - an output tile is one quantization group -, tokens or outs above 2^31 - 1,
 * an LDS image above 160 KiB), tokens == 0 or outs == 0 (FPQ_OK), then NULL pointers / alignment (FPQ_ERR_ARG; codes, out and
 * gelu_out 16 bytes, bias and nan_flag 8).  Tilings as fpq_gemm_a6w4_mx (FPQ_GEMM_CFG 20 / 30 forces one); both give the same bits. */
int fpq_gemm_a6w4_gelu_dual(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes,
                            const void* w_scales, int w_scale_dtype, const void* bias, void* out, void* gelu_out,
                            int64_t tokens, int64_t outs, int64_t k, void* nan_flag, fpq_stream_t stream);

/* THE A6W4 PATH ON K-MAJOR IMAGES ("K-MAJOR OPERAND IMAGES" above) - same arithmetic, same results bit for bit as the three row-major
 * entry points (tests/test_gpu_a6w4_km.py):
 *   activation codes   the activation side's 6-bit image [k / 128][rows][96] (chunk order c = (p - ((j >> 3) & 1)) mod 6, no row
 *                      padding): what fpq_codes_to_kmajor(code_bits = 6, dealt = 0) makes of fpq_quant_rows_codes_g6's codes
 *   activation scales  the fp32 k-major scale image [k / 128][rows rounded up to 4], padding 0
 *   weights            exactly what fpq_gemm_fp4_mx_km takes: the dealt 4-bit image (rows rounded up to 64) and the fp32 weight-side
 *                      scale image - one stored k-major FP4 weight serves both GEMMs, as the row-major one does
 * fpq_a6w4_quant_rows_codes_km: fpq_quant_rows_codes_g6 writing the two activation images directly (padding rows of the scale image
 * are not written).  fp16 rows only (fp32 rows: fpq_quant_rows_codes_g6 + fpq_codes_to_kmajor + fpq_scales_to_kmajor).  Checks, in
 * this order: negative sizes (FPQ_ERR_ARG), table_id (FPQ_ERR_TABLE), in_dtype other than FPQ_F16 (FPQ_ERR_DTYPE), cols % 128 or an
 * image of 2 GiB or more (FPQ_ERR_SHAPE), rows == 0 or cols == 0 (FPQ_OK), then NULL pointers / x, image or scales not 16-byte
 * aligned (FPQ_ERR_ARG).
 * fpq_gemm_a6w4_mx_km / fpq_gemm_a6w4_gelu_dual_km: fpq_gemm_a6w4_mx / fpq_gemm_a6w4_gelu_dual on those images; bias, out, epilogue,
 * gelu_out, nan_flag unchanged.  Checks, in this order, before any launch: a_table (FPQ_ERR_TABLE), negative sizes (FPQ_ERR_ARG),
 * [_mx_km: the epilogue descriptor (FPQ_ERR_ARG)], w_scale_dtype other than FPQ_F32 (FPQ_ERR_DTYPE: the scale images are fp32), shape
 * (FPQ_ERR_SHAPE: the row-major entry point's rules - k % 128, k > 8192, outs % 8 resp. outs % 128, an LDS image above 160 KiB -, then
 * tokens or outs at or above 2^28: the scale images are addressed by 32-bit lane offsets), tokens == 0 or outs == 0 (FPQ_OK), then
 * NULL pointers / alignment (FPQ_ERR_ARG; images, out and gelu_out 16 bytes, bias and nan_flag 8, both scale images 16).  The weight
 * image has outs rounded up to 64 rows.  Tilings as fpq_gemm_a6w4_mx (FPQ_GEMM_CFG 20 / 30 forces one); both give the same bits. */
int fpq_a6w4_quant_rows_codes_km(const void* x, uint8_t* image, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                               fpq_stream_t stream);
int fpq_gemm_a6w4_mx_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                        int w_scale_dtype, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                        const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
int fpq_gemm_a6w4_gelu_dual_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image,
                               const void* w_scales, int w_scale_dtype, const void* bias, void* out, void* gelu_out,
                               int64_t tokens, int64_t outs, int64_t k, void* nan_flag, fpq_stream_t stream);

/* MAT_QKV ON THE A6W4 GEMM: fpq_gemm_a6w4_mx (kmajor = 0) / fpq_gemm_a6w4_mx_km (kmajor = 1) - exactly that entry point's operands
 * and every one of its operand and scale checks, no gate / residual tail - with the SPLIT OUTPUT of fpq_gemm_fp4_mx_split, and
 * with the Q / K L2 NORM above in that epilogue (the mixed W4A4 model's mat_qkv has an E3M0 activation in almost every block).
 * Without the norm every written value is bit for bit the one fpq_gemm_a6w4_mx / _km writes at that (token, column); with it, y16
 * is what they write with bias == NULL and q, k, v follow "THE Q / K L2 NORM" (the arithmetic of fpq_gemm_fp4_mx_split_qknorm:
 * q and k within that section's bound, its non-finite rule, v bit for bit).  Row-major and k-major operands, and both tilings, give the same bits.
 * w_scale_dtype: FPQ_F32 ONLY, row-major operands included - these forms are not compiled for fp16 weight scales (what
 * fpq_quant_rows_codes_mx writes for an fp32 weight, and what the k-major scale images are, is fp32): FPQ_F16 is FPQ_ERR_DTYPE.
 * split: the FP6 family's rules (fpq_gemm_fp6_rows_split) - n_parts 1..3 (exactly 3 with the norm), part_cols % 128 == 0,
 * outs == n_parts * part_cols, rows_per_batch >= 1 and tokens % rows_per_batch == 0; EVERY destination out[p] non-NULL and 8-byte
 * aligned, row_stride[p] >= part_cols and % 4 == 0, batch_stride[p], row0[p] >= 0.  bias: fp16 [outs], 8-byte aligned, or NULL
 * (split); fp32 [3 * part_cols], 16-byte aligned, or NULL (norm); q_head_scale fp32 [part_cols / 64], never NULL.
 * Checks, in this order, before any launch: a_table (FPQ_ERR_TABLE); split == NULL [_qknorm: or n_parts != 3, q_head_scale NULL or
 * not 4-byte aligned, bias not 16-byte aligned] (FPQ_ERR_ARG); negative sizes (FPQ_ERR_ARG); the split descriptor (FPQ_ERR_ARG);
 * w_scale_dtype other than FPQ_F32 (FPQ_ERR_DTYPE); shape (FPQ_ERR_SHAPE: k % 128, k > 8192, tokens or outs above 2^31 - 1, with
 * kmajor tokens or outs at or above 2^28, an LDS image above 160 KiB); tokens == 0 (FPQ_OK, nothing launched); then NULL pointers /
 * alignment (FPQ_ERR_ARG; codes or images 16 bytes, the fp16 bias 8, with kmajor both scale images 16).
 * Tilings as fpq_gemm_a6w4_mx (FPQ_GEMM_CFG 20 / 30 forces one). */
int fpq_gemm_a6w4_mx_split(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                           int w_scale_dtype, const void* bias, int64_t tokens, int64_t outs, int64_t k, const fpq_gemm_split_t* split,
                           int kmajor, fpq_stream_t stream);
int fpq_gemm_a6w4_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                  int w_scale_dtype, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                  const fpq_gemm_split_t* split, const float* q_head_scale, int kmajor, fpq_stream_t stream);

/* ---- W6: E1M2 / E3M0 WEIGHTS as 6-bit codes x an E2M1 / E1M2 / E3M0 activation, per group of 128 --------------------------------
 * The FP4 format search chooses a weight format per layer among E1M2, E2M1 and E3M0; fpq_gemm_fp4_mx and fpq_gemm_a6w4_mx run the
 * E2M1 weights.  fpq_gemm_w6_mx runs the other two: out[t, o] = fp16(bias[o] + sum_g a_scale[t,g] * w_scale[o,g] * dot_128(level(a)[t,g,:],
 * level(w)[o,g,:])), with the optional gate / residual tail of fpq_gemm_epilogue_t (NULL: none).
 *   w_codes   dense 6-bit codes [outs, 3 k / 4] of w_table - FPQ_E1M2 (decoded as FP6 E2M3, blgp = 2) or FPQ_E3M0 (as BF6 E3M2, blgp = 3) -
 *             and w_scales fp32 [outs, k / 128]: exactly what fpq_quant_rows_codes_g6 writes for an fp32 weight.  w_scale_dtype: FPQ_F32
 *             ONLY - the kernels are not compiled for fp16 weight scales (FPQ_F16 is FPQ_ERR_DTYPE, as in the A6W4 split forms).
 *   a_codes   of a_table: FPQ_E2M1 - nibbles [tokens, k / 2] as fpq_quant_rows_codes_mx writes them (cbsz = 4); FPQ_E1M2 / FPQ_E3M0 - 6-bit
 *             codes [tokens, 3 k / 4] as fpq_quant_rows_codes_g6 writes them (cbsz = 2 / 3); a_scales fp16 [tokens, k / 128] in all three.
 * Row-major operands here; the fc1 tail and the split output: fpq_gemm_w6_gelu_dual, fpq_gemm_w6_mx_split / _split_qknorm below; every
 * form on k-major images: the _km twins behind them ("THE W6 GEMM ON K-MAJOR IMAGES").
 * Checks, in this order, before any launch (fpq_gemm_a6w4_mx's order): a_table, w_table (FPQ_ERR_TABLE); negative sizes (FPQ_ERR_ARG); the
 * epilogue descriptor (FPQ_ERR_ARG); w_scale_dtype other than FPQ_F32 (FPQ_ERR_DTYPE); shape (FPQ_ERR_SHAPE: k % 128, k > 8192, outs % 8,
 * tokens or outs above 2^31 - 1, an LDS image above 160 KiB); tokens == 0 or outs == 0 (FPQ_OK, nothing launched); then NULL pointers /
 * alignment (FPQ_ERR_ARG; codes and out 16 bytes, bias 8, scales their dtype).  Two tilings (64 x 128 and 128 x 128 tiles, the K order of
 * both the same: bit-equal), chosen as fpq_gemm_a6w4_mx chooses; FPQ_GEMM_CFG 20 / 30 forces one.
 * Numerics: the per-group steps of fpq_gemm_a6w4_mx - t = fl(d_g sa), acc = fma(t, sw, acc), out = fp16(acc + bias).  Per pair
 * (activation x weight), products are multiples of / at most: E2M1 x E1M2 1/8, 10.5; E2M1 x E3M0 1/8, 96; E1M2 x E1M2 1/16, 3.0625; E1M2 x
 * E3M0 and E3M0 x E1M2 1/16, 28; E3M0 x E3M0 1/16, 256 - the exact 128-term dot has at most 20 significant bits and fits fp32.
 * MEASURED on an MI355X before anything else (profiles/w6_dot.txt): with k = 128, unit scales and no bias, dots that are fp16 numbers -
 * the four constructions of fpq_gemm_a6w4_mx's measurement, for a weight table - come out bit for bit for ALL SIX pairs in both tilings
 * (72 runs, none differs; E3M0 x E3M0 included, unlike full-range E3M2 x E3M2 codes: fpq_gemm_f6_rows).  So for every pair the contract is
 * fpq_gemm_fp4_mx's, unchanged: against the float64 product of the decoded operands every element is within 2^-11 |ref| + 2^-25 +
 * (1 + 2^-10) 2^-24 (S + R + |ref|) (allowance 1.0; worst measured over the shape sweep 1.000 x the bound, the fp16 output rounding), and
 * the output is bit-equal to an fp32 model of those steps (tests/w6_model.py, tests/test_gpu_w6.py). */
int fpq_gemm_w6_mx(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                   int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                   const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
/* fpq_gemm_w6_gelu_dual: fpq_gemm_a6w4_gelu_dual for a 6-bit weight - fc1 of the FFN, its GELU(tanh) and fc2's dual E1M2- / E2M1+
 * per-group(128) input quantizer in ONE launch (+ the NaN fix-up launch): out = fp16 [tokens, outs] =
 * fp_quant_e1m2_neg_e2m1_pos_per_group_cuda(gelu_tanh(y), 4, 128) with y the fp16 [tokens, outs] that fpq_gemm_w6_mx writes for the same
 * operands and bias, bit for bit.  Operands (a_codes, a_scales, a_table, w_codes, w_scales, w_scale_dtype, w_table, bias) exactly
 * fpq_gemm_w6_mx's; the tail, gelu_out (NULL, or fp16 [tokens, outs], 16-byte aligned: the GELU values the quantizer saw) and nan_flag
 * (NULL, or the 8-byte zeroed scratch of fpq_quant_rows_dual) exactly fpq_gemm_fp4_gelu_dual's - the same GELU of the same fp16 value
 * and the same quantizer arithmetic, so the three fc1 entry points agree bit for bit wherever their Linear outputs do.
 * Checks, in this order, before any launch: a_table, w_table (FPQ_ERR_TABLE), negative sizes (FPQ_ERR_ARG), w_scale_dtype other than
 * FPQ_F32 (FPQ_ERR_DTYPE), shape (FPQ_ERR_SHAPE: k % 128, k > 8192, outs % 128 - an output tile is one quantization group -, tokens or
 * outs above 2^31 - 1, an LDS image above 160 KiB), tokens == 0 or outs == 0 (FPQ_OK), then NULL pointers / alignment (FPQ_ERR_ARG; codes,
 * out and gelu_out 16 bytes, bias and nan_flag 8, scales their dtype).  Tilings as fpq_gemm_w6_mx; both give the same bits. */
int fpq_gemm_w6_gelu_dual(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                          int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                          int64_t k, void* nan_flag, fpq_stream_t stream);
/* MAT_QKV ON THE W6 GEMM: fpq_gemm_w6_mx's operands and every one of its operand and scale checks, no gate / residual tail, with the
 * SPLIT OUTPUT of fpq_gemm_fp4_mx_split, and with the Q / K L2 NORM above in that epilogue - fpq_gemm_a6w4_mx_split / _split_qknorm for
 * a 6-bit weight.  Without the norm every written value is bit for bit the one fpq_gemm_w6_mx writes at that (token, column); with it,
 * y16 is what it writes with bias == NULL and q, k, v follow "THE Q / K L2 NORM" (the arithmetic of fpq_gemm_fp4_mx_split_qknorm: q and k
 * within that section's bound, its non-finite rule, v bit for bit).  Row-major operands: there is no kmajor argument (k-major images
 * have entry points of their own, fpq_gemm_w6_mx_split_km / _split_qknorm_km below).  split, bias,
 * q_head_scale: the rules of fpq_gemm_a6w4_mx_split (whole batch entries; every destination 8-byte aligned).
 * Checks, in this order, before any launch: a_table, w_table (FPQ_ERR_TABLE); split == NULL [_qknorm: or n_parts != 3, q_head_scale NULL
 * or not 4-byte aligned, bias not 16-byte aligned] (FPQ_ERR_ARG); negative sizes (FPQ_ERR_ARG); the split descriptor (FPQ_ERR_ARG);
 * w_scale_dtype other than FPQ_F32 (FPQ_ERR_DTYPE); shape (FPQ_ERR_SHAPE: k % 128, k > 8192, outs % 8, tokens or outs above 2^31 - 1, an
 * LDS image above 160 KiB); tokens == 0 (FPQ_OK, nothing launched); then NULL pointers / alignment (FPQ_ERR_ARG; codes 16 bytes, the fp16
 * bias 8, scales their dtype).  Tilings as fpq_gemm_w6_mx (FPQ_GEMM_CFG 20 / 30 forces one); both give the same bits.
 * FPQ_VERSION is unchanged by these three: look the symbols up. */
int fpq_gemm_w6_mx_split(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                         int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                         const fpq_gemm_split_t* split, fpq_stream_t stream);
int fpq_gemm_w6_mx_split_qknorm(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                const fpq_gemm_split_t* split, const float* q_head_scale, fpq_stream_t stream);

/* THE W6 GEMM ON K-MAJOR IMAGES ("K-MAJOR OPERAND IMAGES" above): the four entry points above with every operand as the image the other
 * matrix-core GEMMs run on by default - same arithmetic, same tilings, same results bit for bit as their row-major twins
 * (tests/test_gpu_w6_km.py); the argument lists are the twins', so there is no kmajor flag on either.
 *   a_image    of a_table: FPQ_E2M1 - the activation side's 4-bit image [k / 128][tokens][64], what fpq_quant_rows_codes_mx_km and the
 *              *_mx_km producers write (fpq_gemm_fp4_mx_km's activation operand); FPQ_E1M2 / FPQ_E3M0 - the activation side's 6-bit image
 *              [k / 128][tokens][96], what fpq_a6w4_quant_rows_codes_km and the A6W4 producers with kmajor = 1 write
 *              (fpq_gemm_a6w4_mx_km's activation operand)
 *   a_scales   the fp32 k-major scale image [k / 128][tokens rounded up to 4], padding 0, in all three formats
 *   w_image    the dealt 6-bit image [k / 128][outs rounded up to 64][96]: fpq_codes_to_kmajor(code_bits = 6, dealt = 1) of
 *              fpq_quant_rows_codes_g6's codes - the layout of fpq_gemm_fp6_rows_km's weight operand
 *   w_scales   the fp32 weight-side scale image [k / 128][outs rounded up to 64]: fpq_scales_to_kmajor(weight_side = 1).  w_scale_dtype:
 *              FPQ_F32 only
 * bias, out, epilogue, gelu_out, nan_flag, split, q_head_scale: unchanged.  Checks: each row-major twin's, in its documented order, with
 * the k-major rules where fpq_gemm_a6w4_mx_km has them - w_scale_dtype other than FPQ_F32 is FPQ_ERR_DTYPE as before; behind the shape
 * rules, tokens or outs at or above 2^28 (FPQ_ERR_SHAPE: the scale images are addressed by 32-bit lane offsets); behind the empty-problem
 * return (FPQ_OK), NULL pointers, then alignment (FPQ_ERR_ARG): both images 16 bytes (out, gelu_out, bias, nan_flag as in the twin) and
 * BOTH scale images 16 bytes.  FPQ_VERSION is unchanged by these four: look the symbols up. */
int fpq_gemm_w6_mx_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                      int w_scale_dtype, int w_table, const void* bias, void* out, int64_t tokens, int64_t outs, int64_t k,
                      const fpq_gemm_epilogue_t* epilogue, fpq_stream_t stream);
int fpq_gemm_w6_gelu_dual_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                             int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                             int64_t k, void* nan_flag, fpq_stream_t stream);
int fpq_gemm_w6_mx_split_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                            int w_scale_dtype, int w_table, const void* bias, int64_t tokens, int64_t outs, int64_t k,
                            const fpq_gemm_split_t* split, fpq_stream_t stream);
int fpq_gemm_w6_mx_split_qknorm_km(const uint8_t* a_image, const void* a_scales, int a_table, const uint8_t* w_image, const void* w_scales,
                                   int w_scale_dtype, int w_table, const float* bias, int64_t tokens, int64_t outs, int64_t k,
                                   const fpq_gemm_split_t* split, const float* q_head_scale, fpq_stream_t stream);

/* ---- GF6: FULL-RANGE FP6 (E2M3 / E3M2) operands with per-group(128) scales, on the A6W4 and W6 GEMMs ----------------------------
 * The reference's per-group 6-bit configuration (--w_bit 6 --a_bit 6, per_group on both sides: fp6_quant_e2m3_per_group_cuda /
 * fp6_quant_e3m2_per_group_cuda) and its mixed siblings W4A6 / W6A4.  No GEMM of its own: in fpq_gemm_a6w4_* and fpq_gemm_w6_* the
 * table argument of a 6-bit operand names the HARDWARE DECODE - FPQ_E1M2 selects FP6 E2M3 (cbsz / blgp = 2), FPQ_E3M0 selects BF6
 * E3M2 (3) - and those kernels never look at which of the 64 codes occur: full-range E2M3 codes are valid operands under FPQ_E1M2
 * and full-range E3M2 codes under FPQ_E3M0, in every form and both layouts.  FPQ_E2M3 / FPQ_E3M2 themselves stay refused there.
 *
 * fpq_gf6_quant_rows_codes: the per-group(128) quantizer on table_id = FPQ_E2M3 or FPQ_E3M2 (anything else: FPQ_ERR_TABLE, decided
 * first) straight to dense 6-bit hardware codes in the bit format of fpq_quant_rows_codes_fp6 / _g6, one scale per group, with the
 * quantization decisions of fpq_quant_rows(table_id, cols = 128).
 *   kmajor = 0: x [rows, cols] F16 or F32 -> codes [rows, cols * 3 / 4], scales [rows, cols / 128] in x's dtype
 *   kmajor = 1: x F16 only (F32: FPQ_ERR_DTYPE; use kmajor = 0 + fpq_codes_to_kmajor + fpq_scales_to_kmajor) -> the activation
 *               side's 6-bit image [cols / 128][rows][96] and the fp32 scale image [cols / 128][rows rounded up to 4] of
 *               fpq_a6w4_quant_rows_codes_km (padding rows of the scale image are not written)
 * For fp16 x, half(level(code) * scale) equals fp6_quant_e2m3_per_group_cuda / fp6_quant_e3m2_per_group_cuda(x, 6, 128) bit for
 * bit; for fp32 x the fp32 product cast to fp16 does (the reference's .to(float16)).  Non-finite and all-zero groups follow
 * fpq_quant_rows_codes_g6's rule: the non-finite maximum travels in the SCALE, every code is a valid code, an all-zero group has
 * scale 0 and code 0 throughout.  Checks, in this order: table_id (FPQ_ERR_TABLE), negative sizes (FPQ_ERR_ARG), in_dtype
 * (FPQ_ERR_DTYPE), cols % 128 or - with kmajor - an image of 2 GiB or more (FPQ_ERR_SHAPE), rows == 0 or cols == 0 (FPQ_OK), then
 * NULL pointers / alignment (FPQ_ERR_ARG; x and codes 16 bytes, scales their dtype, the scale image 16).  It launches the
 * kernels behind fpq_quant_rows_codes_g6 / fpq_a6w4_quant_rows_codes_km with the full tables as data.
 *
 * NUMERICS of full-range operands on the two GEMMs (the steps are unchanged: t = fl(d_g sa), acc = fma(t, sw, acc), out = fp16(acc +
 * bias)).  Per pair (activation x weight) the products are multiples of / at most: E2M3 x E2M1 2^-4, 45; E3M2 x E2M1 2^-5, 168;
 * E2M3 x E1M2 2^-5, 13.125; E2M3 x E3M0 2^-5, 120; E3M2 x E1M2 2^-6, 49; E2M3 x E2M3 2^-6, 56.25; E3M0 x E3M2 2^-6, 448; E2M3 x E3M2
 * 2^-7, 210; E3M2 x E3M2 2^-8, 784 (a pair and its mirror image alike) - so the exact 128-term dot has at most 22 significant bits and
 * fits fp32, but for E3M2 x E3M2 (25).  MEASURED on an MI355X before anything else (profiles/gf6_dot.txt; tools/gf6_dot.py): with
 * k = 128, unit scales and no bias, dots that are fp16 numbers - the largest products cancelling beside a few smallest ones, every
 * level pair alone and 128-fold, the largest product beside 127 small ones - come out bit for bit in both tilings for THIRTEEN of the
 * sixteen pairs, E2M3 x E3M2 (22 bits) among them.  For those the contract is fpq_gemm_fp4_mx's, unchanged: allowance 1.0 x the bound
 * (worst measured over the shape sweep 1.000, the fp16 output rounding), bit-equal to the fp32 model of those steps, both tilings
 * and both layouts bit-equal (tests/gf6_model.py, tests/test_gpu_gf6.py).  The three pairs whose operands are BOTH decoded as BF6
 * E3M2 with a full-range side - E3M0 x E3M2, E3M2 x E3M0, E3M2 x E3M2 - are not exact (the cancelling construction loses 8 steps of
 * the smallest product, although two of them fit fp32 on paper; E3M0 x E3M0 is exact, profiles/w6_dot.txt) and over the shape sweep
 * reach 290, 380 and 660 x the bound (profiles/gf6_gemm_bound.txt), far past the 8 x this project grants E3M2 levels on the
 * instruction elsewhere: the C entry points run them like any other codes, the Python layer (gemm.linear_g6*) refuses them.
 * THE FC1 TAIL with full-range codes: fpq_gemm_a6w4_gelu_dual_pair / fpq_gemm_w6_gelu_dual_pair below, for fc2's 4-bit dual pair
 * and for the 6-bit configuration's own (INT- / E2M3+). */
int fpq_gf6_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int table_id, int in_dtype,
                             int kmajor, fpq_stream_t stream);

/* ---- PACKED WEIGHTS <-> WEIGHT OPERANDS (fpqvar_amd/packed.py; csrc/fpq_packed_operands.h) -------------------------------------
 * A packed file stores, per weight, the INDEX of each element's level in the sorted, de-duplicated value table; the matrix-core GEMMs
 * take the level's HARDWARE CODE.  The two differ by a fixed map per field and a layout - no arithmetic on values, no second
 * quantization decision - and each direction is ONE launch, padding included.
 *   packed side   codes: FP4 tables (FPQ_E2M1, FPQ_E1M2, FPQ_E3M0) two index nibbles per byte, element 2i in the low nibble,
 *                 [outs, k / 2]; FP6 tables (FPQ_E2M3, FPQ_E3M2) four 6-bit indices per three bytes, the little-endian bit string
 *                 of fpq_quant_rows_codes_fp6 (packed.pack6), [outs, k * 3 / 4].  scales: one per quantization row - [outs, k / 128]
 *                 with cols == 128, [outs] with cols == k; scale_dtype FPQ_F16 or FPQ_F32 (forward), fp32 (inverse).
 *   operand side  FPQ_E2M1: OCP E2M1 nibbles, [outs, k / 2] (fpq_gemm_fp4_mx's w_codes).  FPQ_E1M2: its levels as FP6 E2M3 codes,
 *                 FPQ_E3M0: as BF6 E3M2 codes, FPQ_E2M3 / FPQ_E3M2: sign-magnitude 6-bit codes - all dense, [outs, k * 3 / 4], the
 *                 form of fpq_quant_rows_codes_g6.  A zero level is code 0 in every format.  Scales always fp32.
 *   the map       index i, zero index Z (7 or 31): magnitude |i - Z|, sign set below Z; code = sign bit | magnitude (E2M1, E2M3,
 *                 E3M2), | magnitude << 1 (E1M2 in E2M3), | magnitude << 2 (E3M0 in E3M2).  The index no table has (nibble 15, field
 *                 63) -> code 0.  Inverse: magnitude = (code >> shift) & Z, index = Z -/+ magnitude: a negative zero gives Z, a code
 *                 that is no level of the table some index in 0 .. 2 Z.
 *   kmajor == 0   row-major w_codes and, per group, w_scales float [outs, k / 128]
 *   kmajor == 1   the dealt weight image [k / 128][outs rounded up to 64][64 | 96], byte for byte fpq_codes_to_kmajor(.., dealt = 1) of
 *                 the row-major codes, and per group the fp32 weight-side scale image of fpq_scales_to_kmajor(.., weight_side = 1);
 *                 the padding rows of both are WRITTEN (zero) by the same launch - the caller need not clear anything.
 *   cols == k     (per channel; FP6 tables only, unless k == 128) the scale vector is not part of the operand layout: scales and
 *                 w_scales are ignored, pass NULL.
 * Checks, in this order, before any launch: table_id outside the five tables (FPQ_ERR_TABLE); negative outs / k / cols
 * (FPQ_ERR_ARG); scale_dtype (FPQ_ERR_DTYPE; the inverse has none); k % 128 != 0, cols neither 128 nor k, cols == k != 128 with an FP4
 * table, or an operand image (rows rounded up to 64, in either layout) of 2 GiB or more (FPQ_ERR_SHAPE); outs == 0 or k == 0
 * (FPQ_OK); NULL pointers or pointers not 16-byte aligned (FPQ_ERR_ARG; the two scale pointers only with cols == 128). */
int fpq_packed_to_operands(const uint8_t* codes, const void* scales, int scale_dtype, uint8_t* w_codes, float* w_scales,
                           int64_t outs, int64_t k, int64_t cols, int table_id, int kmajor, fpq_stream_t stream);
int fpq_operands_to_packed(const uint8_t* w_codes, const float* w_scales, uint8_t* codes, float* scales,
                           int64_t outs, int64_t k, int64_t cols, int table_id, int kmajor, fpq_stream_t stream);

/* THE FC1 TAIL WITH ITS DUAL PAIR AS AN ARGUMENT: fpq_gemm_a6w4_gelu_dual[_km] / fpq_gemm_w6_gelu_dual[_km] with the two tables of fc2's
 * per-group(128) input quantizer (neg_table, pos_table) and the layout (kmajor: 0 row-major operands, else the k-major images of the
 * _km twin) as arguments.  Accepted pairs - anything else FPQ_ERR_TABLE, checked beside the operand tables, before every other check:
 *   (FPQ_E1M2_NEG, FPQ_E2M1_POS)  the 4-bit format: the same launch as the existing entry points, bit for bit, nan_flag included
 *   (FPQ_INT_NEG, FPQ_E2M3_POS)   fc2's format in the per-group 6-bit configuration: out = fp6_quant_int_neg_e2m3_pos_per_group_cuda(
 *                                 gelu_tanh(y), 6, 128) with y the fp16 Linear output of the plain form - bit for bit what
 *                                 fpq_quant_rows_dual / fpq_gelu_quant_rows_dual write for that pair WITHOUT a flag.  This format has no
 *                                 global clamp: a NaN stays out of its group's two maxima (it "belongs to neither side") and comes out
 *                                 as the table's level for a NaN pattern times the scale, the other 127 values are quantized as ever;
 *                                 a +-inf makes its side's scale infinite and, as in the stand-alone kernels, the whole group NaN.
 *                                 nan_flag is checked for alignment like the twin's and otherwise ignored: nothing is raised or zeroed.
 * gelu_out and every other argument, check and tiling: the twins', in the twins' order.  The bucket table behind the scale tiles is
 * sized from the pair (1 KiB for the 4-bit pair, 4 KiB - 2 x 1024 buckets - for the 6-bit one) and counted in the 160 KiB refusal.
 * The 6-bit pair runs kernels of its own (gemm_a6w4_fc1x[_km]_kernel, gemm_w6_fc1x[_km]_kernel: the fc1 kernels with the NaN halves
 * cleared in the values the tail's packed maxima are made of); the kernels behind the existing entry points are untouched. */
int fpq_gemm_a6w4_gelu_dual_pair(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                                 int w_scale_dtype, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs, int64_t k,
                                 void* nan_flag, int neg_table, int pos_table, int kmajor, fpq_stream_t stream);
int fpq_gemm_w6_gelu_dual_pair(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                               int w_scale_dtype, int w_table, const void* bias, void* out, void* gelu_out, int64_t tokens, int64_t outs,
                               int64_t k, void* nan_flag, int neg_table, int pos_table, int kmajor, fpq_stream_t stream);

/* THE PRODUCERS IN FRONT OF THE A6W4 GEMM: the online rotation and the adaLN producer emitting its activation operands in one launch,
 * as fpq_rotate_quant_rows_codes_mx[_km] / fpq_adaln_rotate_quant_rows_codes_mx[_km] do for the FP4 GEMM - the activation never exists
 * in HBM as fp16 between the block's LayerNorm and its matrix product (the mixed W4A4 model's mat_qkv and fc1 have an E3M0 activation
 * in almost every block).  x, rows, cols, in_dtype, smooth, sign_mask_host [, scale, shift, mod_dtype, rows_per_batch, eps]: exactly
 * the arguments of fpq_rotate_quant_rows / fpq_adaln_rotate_quant_rows.  table_id: FPQ_E1M2 or FPQ_E3M0.
 *   kmajor = 0: codes [rows, cols * 3 / 4] (the bit format of fpq_quant_rows_codes_g6), scales fp16 [rows, cols / 128]
 *   kmajor = 1: the activation side's 6-bit image [cols / 128][rows][96] and the fp32 scale image [cols / 128][rows rounded up to 4]
 *               (padding rows not written) - exactly what fpq_gemm_a6w4_mx_km, fpq_gemm_a6w4_gelu_dual_km and the split forms take
 * CONTRACT: let y be the fp16 rotated rows that fpq_rotate_quant_rows / fpq_adaln_rotate_quant_rows write to rotated_out for the same
 * arguments.  Then codes and scales are byte for byte what fpq_quant_rows_codes_g6(y) writes (kmajor = 0) or what
 * fpq_a6w4_quant_rows_codes_km(y) writes (kmajor = 1; padding rows of the scale image excluded).  Hence level(code) * scale equals the
 * `out` of the values form with the same table_id, bit for bit; non-finite groups follow fpq_quant_rows_codes_g6's rule (the maximum
 * itself is the scale, every code is a valid code, an all-zero group has scale 0 and code 0).
 * fpq_a6w4_adaln_rotate_quant_rows_codes runs on the matrix-core kernel only: cols <= 2560 (beyond: FPQ_ERR_SHAPE).
 * Checks, in this order, before any launch: negative sizes, rows_per_batch <= 0 or sign_mask_host == NULL (FPQ_ERR_ARG); table_id
 * (FPQ_ERR_TABLE); in_dtype / mod_dtype other than FPQ_F16 / FPQ_F32 (FPQ_ERR_DTYPE); cols % 128, [adaLN: cols > 2560,] with kmajor an
 * image of 2 GiB or more (FPQ_ERR_SHAPE); rows == 0 or cols == 0 (FPQ_OK, nothing launched); then NULL x / codes / scales [/ scale /
 * shift] or x, codes, scales, smooth [, scale, shift] not 16-byte aligned (FPQ_ERR_ARG). */
int fpq_a6w4_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                     const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor, fpq_stream_t stream);
int fpq_a6w4_adaln_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                           const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                           const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor,
                                           fpq_stream_t stream);

/* THE SAME PRODUCERS ON THE FULL FP6 TABLES (GF6 above): the online rotation and the adaLN producer emitting per-group(128) full-range
 * E2M3 / E3M2 operands in one launch - the activation of a per-group W6A6 / W4A6 mat_qkv or fc1 no longer exists in HBM as fp16 between
 * the block's LayerNorm and its matrix product.  Every argument is its fpq_a6w4_* twin's, in the twin's order; table_id: FPQ_E2M3 or
 * FPQ_E3M2 (the fpq_a6w4_* names keep refusing these two, and these refuse FPQ_E1M2 / FPQ_E3M0 / FPQ_E2M1).
 *   kmajor = 0: codes [rows, cols * 3 / 4] (the bit format of fpq_gf6_quant_rows_codes), scales fp16 [rows, cols / 128]
 *   kmajor = 1: the activation side's 6-bit image [cols / 128][rows][96] and the fp32 scale image [cols / 128][rows rounded up to 4]
 *               (padding rows not written) - what fpq_gemm_a6w4_*_km / fpq_gemm_w6_*_km take under the decode id of the format
 * CONTRACT: let y be the fp16 rotated rows that fpq_rotate_quant_rows / fpq_adaln_rotate_quant_rows write to rotated_out for the same
 * arguments and table_id.  Then codes and scales are byte for byte what fpq_gf6_quant_rows_codes(y, ..., table_id, FPQ_F16, kmajor)
 * writes (padding rows of the scale image excluded), non-finite and all-zero groups included.  Hence level(code) * scale equals the
 * `out` of the values form, bit for bit.
 * The adaLN entry point has no kernel of its own: the 6-bit group form of the adaLN kernel stages whatever bucket -> code table it is
 * handed, here the table fpq_gf6_quant_rows_codes stages (2 x 512 buckets for E2M3, 2 KiB per workgroup).  The rotate entry point
 * takes its codes from the FP6 conversion hardware instead (v_cvt_scalef32_2xpk16_{fp6,bf6}_f32: no table, no staging barrier, the
 * short-workgroup grid of the table-free E2M1 forms) - the same bytes, checked against the table form in tests/test_gpu_gf6_producers.py;
 * the switch FPQ_NO_HW6 = 1 keeps the staged table there too, on the kernel of fpq_a6w4_rotate_quant_rows_codes.
 * fpq_gf6_adaln_rotate_quant_rows_codes runs on the matrix-core kernel only: cols <= 2560 (beyond: FPQ_ERR_SHAPE).
 * Checks, in this order, before any launch: negative sizes, rows_per_batch <= 0 or sign_mask_host == NULL (FPQ_ERR_ARG); table_id
 * (FPQ_ERR_TABLE); in_dtype / mod_dtype other than FPQ_F16 / FPQ_F32 (FPQ_ERR_DTYPE); cols % 128, [adaLN: cols > 2560,] with kmajor an
 * image of 2 GiB or more (FPQ_ERR_SHAPE); rows == 0 or cols == 0 (FPQ_OK, nothing launched); then NULL x / codes / scales [/ scale /
 * shift] or x, codes, scales, smooth [, scale, shift] not 16-byte aligned (FPQ_ERR_ARG).
 * Additions that change no existing entry point: FPQ_VERSION stays, a caller looks the symbols up. */
int fpq_gf6_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                    const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor, fpq_stream_t stream);
int fpq_gf6_adaln_rotate_quant_rows_codes(const void* x, uint8_t* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                          const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                          const float* smooth, const uint32_t* sign_mask_host, int table_id, int kmajor,
                                          fpq_stream_t stream);

/* THE GATED RESIDUAL FOLDED INTO THE adaLN PRODUCER THAT FOLLOWS IT.  In a block every x = x + y.mul(gate) whose y comes out of a GEMM that
 * has no epilogue of ours is followed by an adaLN producer that reads the row just written.  These four run both in one launch:
 *     x_new = residual + y.mul(gate)          written to x_out, [rows, cols] of in_dtype
 *     ...   = the twin entry point on x_new   (fpq_adaln_rotate_quant_rows, _rows_codes_mx[_km], _token_rows, _token_rows_codes_f6)
 * y: fp16 [rows, cols]; gate: fp16 [rows / rows_per_batch, cols], one row per batch entry as scale and shift; residual: the twin's x.
 * Every other argument is the twin's, in the twin's order; kmajor selects the twin's _km form where it has one.
 * CONTRACT (bit equality, no tolerance): x_out is what torch computes on the GPU for residual + y.mul(gate) - fp16 rows:
 * half(residual + half(y * gate)), which is also fpq_gate_residual's result; fp32 rows: residual + float(half(y * gate)) - and every
 * other output is byte for byte what the twin writes when handed x_out as its x.  The same kernel variant runs as for the twin (they
 * share one dispatch), under the same switches.
 * ALIASING: x_out may be exactly `residual` (an in-place residual stream: a row is read and written by one wavefront, and read first).
 * x_out must not overlap y, and must not overlap residual in any other way.
 * Checks: the twin's own come first, in the twin's order (rows == 0 or cols == 0 among them: FPQ_OK, nothing launched); then y, gate or
 * x_out NULL (FPQ_ERR_ARG); y, gate or x_out not 16-byte aligned (FPQ_ERR_ARG); cols > 2560 (FPQ_ERR_SHAPE: the kernel for wider rows
 * has no fused form).  The 6-bit group forms (_g6, _gf6) and the FP8 form have no fused twin.
 * Additions that change no existing entry point: FPQ_VERSION stays, a caller looks the symbols up. */
int fpq_resid_adaln_rotate_quant_rows(const void* y, const void* gate, void* x_out, const void* residual, void* out, void* h_out,
                                      void* rotated_out, int64_t rows, int64_t cols, int in_dtype, const void* scale,
                                      const void* shift, int mod_dtype, int64_t rows_per_batch, float eps, const float* smooth,
                                      const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);
int fpq_resid_adaln_rotate_quant_rows_codes_mx(const void* y, const void* gate, void* x_out, const void* residual, uint8_t* codes,
                                               void* scales, int64_t rows, int64_t cols, int in_dtype, const void* scale,
                                               const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                               const float* smooth, const uint32_t* sign_mask_host, int kmajor, fpq_stream_t stream);
int fpq_resid_adaln_rotate_quant_token_rows(const void* y, const void* gate, void* x_out, const void* residual, void* out,
                                            void* h_out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols,
                                            int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                            int64_t rows_per_batch, float eps, const float* smooth,
                                            const uint32_t* sign_mask_host, int table_id, fpq_stream_t stream);
int fpq_resid_adaln_rotate_quant_token_rows_codes_f6(const void* y, const void* gate, void* x_out, const void* residual,
                                                     uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                                     const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch,
                                                     float eps, const float* smooth, const uint32_t* sign_mask_host, int table_id,
                                                     int kmajor, fpq_stream_t stream);

/* THE SQUARED-ERROR FORMS OF THE MATRIX-CORE GEMMS (the format search's loss, computed where the product is).  Each computes the
 * product as its family's plain row-major entry point does - fpq_gemm_fp4_mx, fpq_gemm_a6w4_mx, fpq_gemm_w6_mx, fpq_gemm_f6_rows
 * (kmajor = 0), no gate / residual tail - but writes no output tensor.  Its result is one float:
 *     y16[t, o] = bit for bit what that entry point stores for the same operands and bias
 *     *loss_out = sum_t row_weight[t] * sum_o ( f32(ref[t, o]) - f32(y16[t, o]) )^2
 * i.e. fpq_sqerr_rows_weighted(ref, y16, row_weight) with one plane, without y16's trip through memory.
 * Arguments: the family's plain entry point up to `bias`, then
 *   ref         [tokens, outs] contiguous, `ref_dtype` FPQ_F16 or FPQ_F32, 16-byte aligned
 *   row_weight  float32 [tokens], FINITE AND POSITIVE, 16-byte aligned
 *   loss_out    one float32, overwritten (not accumulated), 4-byte aligned
 *   workspace   at least fpq_gemm_sqerr_workspace_bytes(tokens, outs) bytes of device scratch, 4-byte aligned: 4 bytes per
 *               64 x 128 tile, the smallest tiling any family launches, and never less than 4 (a negative or > 2^31 - 1 size: FPQ_ERR_ARG)
 *   tokens, outs, k, stream.
 * The operands are row-major codes and scales; k-major images are not taken by these four.  Each launch uses the tiling the family's rule picks for the plain form
 * (FPQ_GEMM_CFG 20 / 30, for the FP4 family 10 too, and FPQ_GEMM6_CFG force one as there); the FP4 family's deep ring (40) and its
 * register-staged kernels have no such form: 40 runs the 64 x 128 tile (30, the same bits), and what only the register-staged
 * kernel serves - a bias that is not 8-byte aligned (FPQ_ERR_ARG), a K whose scale tiles fit no LDS image (FPQ_ERR_SHAPE) - is refused.
 * Two launches: the GEMM, whose workgroups leave one fp32 partial per tile (the differences, squares and sums in fp32, the
 * wavefronts' butterfly, the four wavefronts in order), and one workgroup that adds the partials in a fixed order
 * (fpq_sqerr_rows_weighted's second kernel).  No atomics, no memset: the same inputs give the same bits on every call whatever
 * the workspace held; no host synchronisation, allocation or copy - legal inside a stream capture.
 * Checks, before anything is enqueued: the family's own come first, in the family's order and with its codes (`out` is not
 * among them); then loss_out or workspace NULL or not 4-byte aligned, ref or row_weight NULL or not 16-byte aligned
 * (FPQ_ERR_ARG); then ref_dtype (FPQ_ERR_DTYPE).  tokens == 0 or outs == 0 - where the family returns FPQ_OK - stores 0.0f with
 * one launch and returns FPQ_OK; ref and row_weight are not looked at then.
 * Accuracy: every term is non-negative and every weight positive, so against the exact sum S of the stored ref, y16 and weights
 *   |*loss_out - S| <= ((1 + 2^-24)^(D + c) - 1) S,    D = 4 MT + ceil(tiles / 256) + 22,  c = 3
 * MT = the tile's rows / 32 (2, 4 or 8: a lane holds 4 MT rows), tiles = ceil(tokens / (32 MT)) ceil(outs / 128).  The chain: 4
 * additions over a lane's four outputs of a row, 4 MT over its rows, 6 + 3 in the workgroup, ceil(tiles / 256) + 6 + 3 over the
 * partials; c = the roundings of the difference, the square and the weight.  [13600 x 5760] at 128-row tiles: D + c = 60,
 * 3.6e-6.  FPQ_F16 ref: nothing goes subnormal (the smallest non-zero difference squared is 2^-48), a zero loss is met exactly;
 * FPQ_F32 ref adds at most 2^-149 per element and per row of a lane.
 * Non-finite inputs behave as the fp32 expression does (fpq_sqerr_rows_weighted): the loss is NaN if any counted difference is
 * NaN, otherwise +inf if any is infinite.  Rows t >= tokens and columns o >= outs of an edge tile are not counted, whatever the
 * clamped duplicates in their place hold.
 * Additions that change no existing entry point: FPQ_VERSION stays, a caller looks the symbols up. */
int64_t fpq_gemm_sqerr_workspace_bytes(int64_t tokens, int64_t outs);
int fpq_gemm_fp4_sqerr(const uint8_t* a_codes, const void* a_scales, const uint8_t* w_codes, const void* w_scales, int w_scale_dtype,
                       const void* bias, const void* ref, int ref_dtype, const float* row_weight, float* loss_out, void* workspace,
                       int64_t tokens, int64_t outs, int64_t k, fpq_stream_t stream);
int fpq_gemm_a6w4_sqerr(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                        int w_scale_dtype, const void* bias, const void* ref, int ref_dtype, const float* row_weight, float* loss_out,
                        void* workspace, int64_t tokens, int64_t outs, int64_t k, fpq_stream_t stream);
int fpq_gemm_w6_sqerr(const uint8_t* a_codes, const void* a_scales, int a_table, const uint8_t* w_codes, const void* w_scales,
                      int w_scale_dtype, int w_table, const void* bias, const void* ref, int ref_dtype, const float* row_weight,
                      float* loss_out, void* workspace, int64_t tokens, int64_t outs, int64_t k, fpq_stream_t stream);
int fpq_gemm_f6_rows_sqerr(const uint8_t* a_codes, const void* a_scales, int a_scale_dtype, int a_table, const uint8_t* w_codes,
                           const void* w_scales, int w_scale_dtype, int w_table, const void* bias, const void* ref, int ref_dtype,
                           const float* row_weight, float* loss_out, void* workspace, int64_t tokens, int64_t outs, int64_t k,
                           fpq_stream_t stream);

/* fpq_kv_cache_step_qknorm: fpq_kv_cache_step (same arguments, same checks) for an fp16 qkv WITHOUT the norm (path F, or a
 * mat_qkv that is not split): the new k is normalized and the bias added on its way into the cache, and the same launch writes
 * q_out - fp16 [batch, n_new, row_elems], contiguous - from new_q (the pitches of new_k).  head_dim == 64, row_elems % 64 == 0,
 * group 64 or 128; q_head_scale fp32 [row_elems / 64] never NULL; bias fp32 [3 * row_elems] (q, k, v) 16-byte aligned or NULL;
 * new_q / q_out 16-byte aligned.  Anything else: FPQ_ERR_ARG before any launch. */
int fpq_kv_cache_step_qknorm(void* cache, int64_t batch, int64_t max_len, int64_t row_elems, int64_t quant_start,
                             int64_t quant_stop, const void* new_q, const void* new_k, const void* new_v, int64_t new_batch_pitch,
                             int64_t new_token_pitch, int64_t new_start, int64_t n_new, int64_t group, int table_id,
                             void* q_out, const float* q_head_scale, const float* bias, int64_t head_dim, fpq_stream_t stream);

/* Inverse of fpq_quant_rows_codes: out = (Tout)((float)table_dedup[code] * (float)scale). */
int fpq_dequant_rows_codes(const uint8_t* codes, const void* scales, void* out, int64_t rows,
                           int64_t cols, int table_id, int scale_dtype, int out_dtype,
                           int pack_nibbles, fpq_stream_t stream);

/* The two above over many tensors in ONE launch each: the packed exchange format of the sharded weight calibration
 * (every Linear a rank owns -> nibble codes + one scale per group straight into its slot of the all-gather slab; after
 * the gather every rank decodes all layers of all ranks; reference: quantize_VAR, tr/quant_utils.py:1095-1167 over
 * QuantizedLinear.from_float :828-837, whose result this reproduces bit for bit at 0.53 B per element on the wire).
 * segments_device: DEVICE-resident array of n_segments descriptors, as for fpq_quant_rows_segments; every segment is
 * `rows` groups of `cols` elements; x / codes / out 16-byte aligned, scales aligned to their dtype; max_rows = the
 * largest segment (sizes grid.x; grid.y = segment).  This version: cols == 128, n_segments <= 65535; scales have
 * in_dtype (quantize) / scale_dtype (decode).  Same results as the single-tensor calls per segment.  The descriptors'
 * pointers are NOT validated (they live on the device): the caller guarantees them. */
typedef struct {
  const void* x;
  uint8_t* codes;
  void* scales;
  int64_t rows;
} fpq_codes_segment_t;
int fpq_quant_rows_codes_segments(const fpq_codes_segment_t* segments_device, int n_segments, int64_t max_rows,
                                  int64_t cols, int table_id, int in_dtype, int pack_nibbles, fpq_stream_t stream);
typedef struct {
  const uint8_t* codes;
  const void* scales;
  void* out;
  int64_t rows;
} fpq_decode_segment_t;
int fpq_dequant_rows_codes_segments(const fpq_decode_segment_t* segments_device, int n_segments, int64_t max_rows,
                                    int64_t cols, int table_id, int scale_dtype, int out_dtype, int pack_nibbles,
                                    fpq_stream_t stream);

/* FULL-WIDTH online rotation fused in front of the per-group(128) quantizer: the online side of the reference's `--rotate`
 * without `--block_rotate` (rotate_utils/rotation_utils.py:57-63: Q = diag(D) . H_cols^T / sqrt(cols), H_cols = hadK (x)
 * Sylvester(cols / K)), where
 *     x1 = torch.matmul(producer.mul(s), Q)            tr/basic_var.py:263,266 (fp16 autocast): a dense [rows x cols] . [cols x cols]
 *     q  = fp_quant_e{1,2,3}_per_group_cuda(x1, 4, 128) / fp6_quant_*_per_group_cuda
 * becomes one launch:  h = half(x * s);  y = half(c_h * sum_j +-h_j) with the signs of diag(D) . H_cols^T and
 * c_h = float(half(float32(1 / sqrt(cols)))), the one magnitude of half(float32(Q));  out = per-group(128) quant(y).
 * Both Hadamard factors run on the matrix cores, 2 cols (K + cols / K) FLOP per row (csrc/fpq_fullrot.h: the one row loop of every
 * fpq_fullrot_* entry point; csrc/fpq_fullrot_launch.h: their checks and the launch).
 * Built widths: cols == 1920 (had60 x 2^5) and cols == 2304 (had36 x 2^6).  EVERY other width - the powers of two, 1280 and 1536
 * included - is FPQ_ERR_SHAPE.
 * x: [rows, cols] F16 or F32; smooth: device float[cols] or NULL;
 * sign_words_host: HOST pointer to cols / 32 x uint32, bit j set <=> D[j] == -1, D the cols-long vector of seed 42 (NOT the 128
 * signs of the block form tiled);
 * out: fp16 [rows, cols]; rotated_out: NULL, or fp16 [rows, cols] receiving y; table_id: every symmetric table.
 * Parity: out == fpq_quant_rows(y) bit for bit.  y: the +-h_j are summed in fp32 on the matrix cores (the intermediate between
 * the two factors enters the second as three bf16 pieces that add up to it exactly), at most cols / K + 3 K - 1 roundings of
 * partial sums:  |y - exact| <= 1/2 fp16 ulp (1 + 2^-11) + (cols / K + 3 K - 1) 2^-24 c_h sum|h_j|  (tests/fullrot_model.py).
 * A non-finite input poisons its whole row, as in the reference (the dense Q has no zero entry); y is +-inf exactly where the
 * exact product overflows fp16 or is infinite, with its sign.
 * Checks, in this order, before any launch: rows < 0, cols < 0 or sign_words_host NULL (FPQ_ERR_ARG); table_id (FPQ_ERR_TABLE);
 * in_dtype (FPQ_ERR_DTYPE); cols not a built width or rows >= 2^31 (FPQ_ERR_SHAPE); rows == 0 -> FPQ_OK, nothing is launched;
 * x or out NULL, a pointer not 16-byte aligned (FPQ_ERR_ARG). */
int fpq_fullrot_quant_rows(const void* x, void* out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype,
                           const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream);
/* The same launch emitting the FP4 GEMM's activation operands: what fpq_quant_rows_codes_mx (kmajor == 0: codes uint8 [rows,
 * cols / 2], scales fp16 [rows, cols / 128]) or fpq_quant_rows_codes_mx_km (kmajor != 0: the k-major images, codes [cols / 128,
 * rows, 64], scales fp32 [cols / 128, rows rounded up to 4] - the padding is the caller's) writes for y, byte for byte; F32 rows
 * are taken in both layouts.  Checks: scales NULL with rows > 0 and a built width (FPQ_ERR_ARG), then those of
 * fpq_fullrot_quant_rows (the table is FPQ_E2M1; FPQ_ERR_SHAPE also for a k-major image of 2 GiB or more). */
int fpq_fullrot_quant_rows_codes_mx(const void* x, void* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                    const float* smooth, const uint32_t* sign_words_host, int kmajor, fpq_stream_t stream);

/* The complete producer of tr/basic_var.py:263 / :266 in the FULL-WIDTH mode, one launch: fpq_adaln_rotate_quant_rows' LayerNorm and
 * modulate in front of fpq_fullrot_quant_rows' rotation and quantizer (csrc/fpq_fulladaln.h: the adaLN front of that row loop):
 *     h   = half( ((LayerNorm(x) * half(scale + 1)) + shift) * smooth )    (no affine, eps; the statistics of the raw x in fp32, always
 *                                                                            centred; fp16 modulation adds the 1 in fp16)
 *     y   = half( c_h * sum_j +-h_j )             (= h @ half(Q), Q the full-width matrix)
 *     out = per-group(128) quant(y)
 * x: [rows, cols] F16 / F32, cols == 1920 or 2304 (every other width: FPQ_ERR_SHAPE); scale, shift: [rows / rows_per_batch, cols] in
 * mod_dtype (F16 or F32, both the same), row r takes entry r / rows_per_batch; smooth: device float[cols] or NULL;
 * sign_words_host as in fpq_fullrot_quant_rows; h_out / rotated_out: NULL or fp16 [rows, cols] receiving h / y, each on its own;
 * table_id: every symmetric table.
 * Parity: y and out are fpq_fullrot_quant_rows(h) bit for bit; h is within tests/fulladaln_model.py's bound of the float64 chain (the
 * bound of tests/adaln_model.py with this kernel's summation depth - 8 + 3 + 6 additions at 1920, 8 + 5 + 6 at 2304 - and no one-pass branch).
 * Checks, in this order, before any launch: rows < 0, cols < 0, sign_words_host NULL, rows_per_batch <= 0 or rows not a multiple of
 * rows_per_batch (FPQ_ERR_ARG); table_id (FPQ_ERR_TABLE); in_dtype, mod_dtype (FPQ_ERR_DTYPE); cols not a built width or
 * rows >= 2^31 (FPQ_ERR_SHAPE); rows == 0 -> FPQ_OK, nothing is launched; x, out, scale or shift NULL, a pointer not 16-byte
 * aligned (FPQ_ERR_ARG). */
int fpq_fullrot_adaln_quant_rows(const void* x, void* out, void* h_out, void* rotated_out, int64_t rows, int64_t cols, int in_dtype,
                                 const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                 const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream);
/* The same launch emitting the FP4 GEMM's activation operands, as fpq_fullrot_quant_rows_codes_mx does for y (kmajor == 0: codes
 * uint8 [rows, cols / 2], scales fp16 [rows, cols / 128]; kmajor != 0: the k-major images, the padding of the scale image is the
 * caller's).  Checks: scales NULL with rows > 0 and a built width (FPQ_ERR_ARG), then those of fpq_fullrot_adaln_quant_rows (the
 * table is FPQ_E2M1; FPQ_ERR_SHAPE also for a k-major image of 2 GiB or more). */
int fpq_fullrot_adaln_quant_rows_codes_mx(const void* x, void* codes, void* scales, int64_t rows, int64_t cols, int in_dtype,
                                          const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                          const float* smooth, const uint32_t* sign_words_host, int kmajor, fpq_stream_t stream);

/* Both full-width producers in front of the PER-TOKEN quantizer (W6A6: per-token E2M3 / E3M2 activations, run.sh:7,10,22,25, under
 * `--rotate` without `--block_rotate`): fpq_fullrot_quant_rows' / fpq_fullrot_adaln_quant_rows' launch with
 *     out = fp6_quant_{e2m3,e3m2}_per_token_cuda(y, 6)      ONE scale per row of `cols` channels (tr/quant_utils.py:503-534)
 * behind the rotation instead of the per-group quantizer (csrc/fpq_fulltoken.h: the second tail of that row loop).  The rotated row lies complete in the wavefront's
 * LDS image when the quantizer starts: the row maximum is one pass over that image, no second pass over memory.
 * Arguments as the per-group twins' (x, smooth, sign_words_host, the modulation block) and as the 128-block token forms'
 * (fpq_adaln_rotate_quant_token_rows, _token_rows_codes_f6): row_scales is the last output pointer, fp16 [rows].
 * cols == 1920 or 2304; EVERY other width is FPQ_ERR_SHAPE.  table_id: FPQ_E2M3 or FPQ_E3M2, everything else FPQ_ERR_TABLE.
 * Values forms: out fp16 [rows, cols]; rotated_out, h_out, row_scales: NULL or fp16 [rows, cols] / [rows, cols] / [rows], each on its own.
 * Code forms (the FP6 GEMM's activation operands, fpq_gemm_fp6_rows / fpq_gemm_f6_rows): codes = dense 6-bit codes of table_id,
 * kmajor == 0: uint8 [rows, cols * 3 / 4]; kmajor != 0: the activation side's k-major image [cols / 128, rows, 96] (K-MAJOR OPERAND
 * IMAGES above); row_scales fp16 [rows] in both layouts, required.  Every byte of the `rows` rows is written in either layout; a
 * caller that pads the image's row count for a consumer owns the padding rows.
 * Parity, all bit for bit: y (rotated_out) == fpq_fullrot_quant_rows' y for the same x, smooth and signs; h_out and y behind the
 * adaLN front == fpq_fullrot_adaln_quant_rows' h and y (so both inherit the bounds of tests/fullrot_model.py / tests/fulladaln_model.py);
 * out == fpq_quant_rows(y, cols = row length) and row_scales == that quantizer's scales; (codes, row_scales) ==
 * fpq_quant_rows_codes_f6(y, table_id, kmajor) byte for byte, and level(code) * scale == out.  An all-zero y row gives scale 0 and
 * +0 / code 0 everywhere; a row with a non-finite y gives what the stand-alone quantizer gives on that y; a row's scale depends on
 * no other row.
 * Checks, in this order, before any launch: rows < 0, cols < 0, sign_words_host NULL (adaLN forms: rows_per_batch <= 0 or rows not
 * a multiple of rows_per_batch) (FPQ_ERR_ARG); table_id (FPQ_ERR_TABLE); in_dtype (adaLN forms: mod_dtype) (FPQ_ERR_DTYPE); cols not
 * a built width, rows >= 2^31 or a k-major image of 2 GiB or more (FPQ_ERR_SHAPE); rows == 0 -> FPQ_OK, nothing is launched; x or
 * out (adaLN forms: scale, shift) NULL, a pointer not 16-byte aligned (FPQ_ERR_ARG).  The code forms look at row_scales first: NULL
 * with rows > 0 and a built width is FPQ_ERR_ARG.
 * Additions that change no existing entry point: FPQ_VERSION stays, a caller looks the symbols up. */
int fpq_fullrot_quant_token_rows(const void* x, void* out, void* rotated_out, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                 const float* smooth, const uint32_t* sign_words_host, int table_id, fpq_stream_t stream);
int fpq_fullrot_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                          const float* smooth, const uint32_t* sign_words_host, int table_id, int kmajor,
                                          fpq_stream_t stream);
int fpq_fullrot_adaln_quant_token_rows(const void* x, void* out, void* h_out, void* rotated_out, void* row_scales, int64_t rows,
                                       int64_t cols, int in_dtype, const void* scale, const void* shift, int mod_dtype,
                                       int64_t rows_per_batch, float eps, const float* smooth, const uint32_t* sign_words_host,
                                       int table_id, fpq_stream_t stream);
int fpq_fullrot_adaln_quant_token_rows_codes_f6(const void* x, uint8_t* codes, void* row_scales, int64_t rows, int64_t cols, int in_dtype,
                                                const void* scale, const void* shift, int mod_dtype, int64_t rows_per_batch, float eps,
                                                const float* smooth, const uint32_t* sign_words_host, int table_id, int kmajor,
                                                fpq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FPQ_H */
