/* gemmul8_c.h -- C ABI of the MI355X-native Ozaki-scheme-II GEMM emulator.
 *
 * Plain pointers and sizes only (no C++ / torch types), for ctypes, cgo, JNI or
 * any FFI.  The reference has no C ABI; each entry below replaces one C++ entry
 * point of GEMMul8/include/gemmul8.hpp:
 *
 *   gemmul8_work_size  <- gemmul8::workSize            (gemmul8.hpp:18-22, gemmul8.cu:129-147)
 *   gemmul8_gemm       <- gemmul8::gemm<TA,TB,TC>      (gemmul8.hpp:29-287, gemmul8.cu:149-1316)
 *                         stream instead of hipblasHandle_t, dtype codes instead of template args
 *
 * All device pointers are column-major HIP device memory; alpha/beta are host
 * pointers to one TC value; the work buffer is caller-owned (>= work size).
 * Return codes: 0 ok, GEMMUL8_E_* < 0 on invalid arguments (nothing enqueued).
 * GEMMUL8_E_HIP: a kernel launch of THIS call failed; the phases after it were not enqueued
 * (C is written only by the last phase).  An error left pending on the calling thread by
 * earlier HIP calls is neither reported as the call's own nor cleared (hipGetLastError still
 * returns it to the application).
 */
#ifndef GEMMUL8_C_H
#define GEMMUL8_C_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GEMMUL8_OP_N = 0, GEMMUL8_OP_T = 1, GEMMUL8_OP_C = 2 };
enum { GEMMUL8_R_64F = 0, GEMMUL8_R_32F = 1, GEMMUL8_C_64F = 2, GEMMUL8_C_32F = 3 };
enum { GEMMUL8_REAL_DEFAULT = 0, GEMMUL8_COMPLEX_BIG_MATRIX_ENCODE = 1, GEMMUL8_COMPLEX_CLASSIC_MULT = 2,
       GEMMUL8_COMPLEX_KARATSUBA_MULT = 3 };
enum {
    GEMMUL8_OK = 0,
    GEMMUL8_E_MODULI = -1,       /* num_moduli outside [2, 20] */
    GEMMUL8_E_TYPES = -2,        /* unsupported dtype combination for compute_type */
    GEMMUL8_E_OP = -3,           /* unsupported transpose op */
    GEMMUL8_E_SIZE = -4,         /* padded k beyond 2^22 (fast) / 2^19 - 64 (accurate), or a leading dimension too small */
    GEMMUL8_E_UNSUPPORTED = -5,  /* compute type / mode not implemented on this build */
    GEMMUL8_E_HIP = -6           /* a HIP launch or runtime call failed */
};

/* bytes of workspace required by gemmul8_gemm for this shape (0 for an unknown compute_type).  A function of the
 * shape alone, not of the device.  Shapes of at most 64 output tiles of 256 x 256 and at least 256 k-steps of 64
 * (no Karatsuba sub-products) carry 16 MiB more behind every other area: the partial tiles and arrival counters of
 * the split-K products ("gemm_i8_splitk_kernel"). */
size_t gemmul8_work_size(size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type);

/* C = alpha * op(A) * op(B) + beta * C, emulated with num_moduli int8 products.
 * stream: hipStream_t (NULL = null stream).  fastmode: 1 = vecnorm shifts, 0 = accurate (int8 bound product).
 * phase_ns: optional double[4]; when non-NULL the call waits for its own completion and stores the
 * phase times {scaling, int8 products, conversion (fused: 0), inverse scaling} in nanoseconds. */
int gemmul8_gemm(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b, int type_c,
                 const void *alpha, const void *A, size_t lda, const void *B, size_t ldb, const void *beta, void *C,
                 size_t ldc, unsigned num_moduli, int fastmode, void *work, int compute_type, double *phase_ns);

/* --- low-memory mode ------------------------------------------------------
 * The same product with only `slice_planes` planes of A / B slices resident: the moduli are
 * encoded and multiplied in groups of that size (A and B are re-read once per group).  The
 * result is bit-identical to gemmul8_gemm.  At 8192^3 with 14 moduli the workspace drops from
 * 2.63 GiB to 1.13 GiB with slice_planes = 2.  slice_planes = 0 or >= num_moduli: all resident. */
size_t gemmul8_work_size_lowmem(size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type,
                                unsigned slice_planes);
int gemmul8_gemm_lowmem(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b,
                        int type_c, const void *alpha, const void *A, size_t lda, const void *B, size_t ldb,
                        const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode, void *work,
                        int compute_type, unsigned slice_planes, double *phase_ns);

/* --- strided-batched call ----------------------------------------------------------------------
 * gemmul8_gemm applied to each b in [0, batch) with A + b * stride_a, B + b * stride_b, C + b * stride_c
 * (strides in elements; stride_a or stride_b may be 0: one operand shared by the batch); alpha and beta are one
 * host value for the batch.  Every element's result is bit-identical to gemmul8_gemm on that element.
 * Real f64 operands in fast mode with round_up(k, 64) <= 2048 run ONE split, ONE product and ONE CRT launch for
 * the whole batch (the product kernel reported as "gemm_i8_batched_kernel" / "gemm_i8_batched_onetile_kernel");
 * every other form runs the single-problem phases element by element in the same workspace.
 * The workspace size is for the whole batch and grows linearly with it; callers short of memory split the batch.
 * stride_c < ldc * n with batch > 1 returns GEMMUL8_E_SIZE; gemmul8_gemm's argument checks apply unchanged;
 * batch == 0 returns GEMMUL8_OK; on any error nothing is enqueued.  phase_ns as gemmul8_gemm (the fallback loop
 * sums its elements' phase times). */
size_t gemmul8_work_size_strided_batched(size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type,
                                         size_t batch);
int gemmul8_gemm_strided_batched(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a,
                                 int type_b, int type_c, const void *alpha, const void *A, size_t lda,
                                 size_t stride_a, const void *B, size_t ldb, size_t stride_b, const void *beta, void *C,
                                 size_t ldc, size_t stride_c, size_t batch, unsigned num_moduli, int fastmode,
                                 void *work, int compute_type, double *phase_ns);

/* --- symmetric rank-k update ---------------------------------------------------------------------
 * trans = GEMMUL8_OP_N: C = alpha * A * A^T + beta * C with A n x k; GEMMUL8_OP_T: C = alpha * A^T * A + beta * C
 * with A k x n; column-major.  Only the `uplo` triangle of the n x n C, diagonal included, is read (and only when
 * beta != 0) and written; the other triangle and the ldc padding are never touched.  The triangle carries the
 * same bits as gemmul8_gemm(trans, opposite op, n, n, k, A, A) writes there (BLAS epilogue semantics always:
 * gemmul8_set_epilogue does not apply), and uplo = lower is the transpose of uplo = upper bit for bit.
 * Fast mode splits op(A) once and multiplies the T (T + 1) / 2 tiles of the triangle per modulus (T = n / 256
 * rounded up; "gemm_i8_syrk_kernel" / "gemm_i8_syrk_onetile_kernel"); accurate mode runs gemmul8_gemm's split.
 * Padded k beyond 2^16 runs gemmul8_gemm's products over all tiles; the CRT is triangular either way.
 * Real types only: type_a, type_c in {R_64F, R_32F} as gemmul8_gemm accepts them with type_b = type_a; a complex
 * type returns GEMMUL8_E_TYPES, GEMMUL8_OP_C or an unknown uplo GEMMUL8_E_OP; moduli, size and leading-dimension
 * checks are gemmul8_gemm's; n == 0 returns GEMMUL8_OK; on any error nothing is enqueued.  phase_ns as
 * gemmul8_gemm.  gemmul8_work_size_syrk(n, k, N) == gemmul8_work_size(n, n, k, N, GEMMUL8_REAL_DEFAULT). */
enum { GEMMUL8_FILL_LOWER = 0, GEMMUL8_FILL_UPPER = 1 };
size_t gemmul8_work_size_syrk(size_t n, size_t k, unsigned num_moduli);
int gemmul8_syrk(void *stream, int uplo, int trans, size_t n, size_t k, int type_a, int type_c, const void *alpha,
                 const void *A, size_t lda, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode,
                 void *work, double *phase_ns);

/* --- Hermitian rank-k update ---------------------------------------------------------------------
 * trans = GEMMUL8_OP_N: C = alpha * A * A^H + beta * C with A n x k; GEMMUL8_OP_C: C = alpha * A^H * A + beta * C
 * with A k x n; column-major, complex.  alpha and beta point to one REAL host value of C's precision (double for
 * C_64F, float for C_32F), as in BLAS zherk / cherk.  Only the `uplo` triangle of the n x n C, diagonal included,
 * is read (and only when beta != 0) and written; the other triangle and the ldc padding are never touched.
 * Off the diagonal the triangle carries the bits gemmul8_gemm(trans, opposite op (N <-> C), n, n, k, A, A) writes
 * there with alpha = (alpha, 0), beta = (beta, 0) and any complex compute type (accurate mode:
 * GEMMUL8_COMPLEX_KARATSUBA_MULT or CLASSIC_MULT, whose bound carries no reference defect); BLAS epilogue semantics
 * always (gemmul8_set_epilogue does not apply).  On the diagonal the imaginary part of C is not read and is written
 * as +0.0, and the real part carries gemmul8_gemm's bits for a C whose diagonal imaginary parts are +0.0.  The two
 * `uplo` results are each pinned to gemmul8_gemm's own triangle; that one is the conjugate transpose of the other
 * bit for bit is not promised.
 * The products always run on the Karatsuba geometry: per modulus the T (T + 1) / 2 tiles of the triangle of each
 * of the three sub-products (T = n / 256 rounded up; "gemm_i8_herk_kernel" / "gemm_i8_herk_onetile_kernel").
 * Padded k beyond 2^16 runs gemmul8_gemm's products over all tiles; the CRT is triangular either way.
 * Complex types only: type_a, type_c in {C_64F, C_32F} as gemmul8_gemm accepts them with type_b = type_a; a real
 * type returns GEMMUL8_E_TYPES, GEMMUL8_OP_T or an unknown uplo GEMMUL8_E_OP; moduli, size and leading-dimension
 * checks are gemmul8_gemm's; n == 0 returns GEMMUL8_OK; on any error nothing is enqueued.  phase_ns as
 * gemmul8_gemm.  gemmul8_work_size_herk(n, k, N) is the Karatsuba layout's size at every shape (==
 * gemmul8_work_size(n, n, k, N, GEMMUL8_COMPLEX_KARATSUBA_MULT) wherever gemmul8_gemm takes that geometry). */
size_t gemmul8_work_size_herk(size_t n, size_t k, unsigned num_moduli);
int gemmul8_herk(void *stream, int uplo, int trans, size_t n, size_t k, int type_a, int type_c, const void *alpha,
                 const void *A, size_t lda, const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode,
                 void *work, double *phase_ns);

/* --- triangular matrix multiply --------------------------------------------------------------------
 * side = GEMMUL8_SIDE_LEFT: C = alpha * op(A) * B with A m x m; GEMMUL8_SIDE_RIGHT: C = alpha * B * op(A) with A
 * n x n; op = trans (GEMMUL8_OP_N / OP_T; complex types: also OP_C); B and C m x n; column-major.  A is triangular: only its `uplo` triangle is
 * read, and with GEMMUL8_DIAG_UNIT not its diagonal either, which counts as exactly 1.0; the unreferenced elements
 * never influence the result and may hold anything, NaN and Inf included.  There is no beta (the out-of-place form
 * of rocBLAS / hipBLAS-v2 trmm): C is never read, the CRT runs with beta = 0 under BLAS epilogue semantics
 * (gemmul8_set_epilogue does not apply).
 * In place: C == B is allowed when ldc == ldb and type_c == type_b (BLAS trmm) -- split, products and CRT are
 * ordered on the stream and B is split completely before the CRT writes C.  Any other overlap of C with A or B is
 * undefined.
 * C carries the bits gemmul8_gemm writes with beta = 0 for A's explicit dense form (zeros outside the triangle, ones
 * on a unit diagonal): gemm(trans, N, m, n, m, A, B) on the left, gemm(N, trans, m, n, n, B, A) on the right, in
 * fast and accurate mode and for ragged sizes.
 * The split reads the triangle's half of A only, and the products run every tile over the k-steps its triangle
 * leaves nonzero, (T + 1) / 2T of the full product's (T = tiles of 256 along A; "gemm_i8_trmm_kernel" /
 * "gemm_i8_trmm_onetile_kernel").  Padded k beyond 2^16 runs gemmul8_gemm's products over all tiles.
 * Types: all real, in the combinations gemmul8_gemm accepts for type_a / type_b / type_c under
 * GEMMUL8_REAL_DEFAULT, or all complex (below); a mix of real and complex types returns GEMMUL8_E_TYPES;
 * GEMMUL8_OP_C with real types or an unknown side / uplo / diag GEMMUL8_E_OP; moduli, size and leading-dimension
 * checks are gemmul8_gemm's (lda >= m on the left, >= n on the right; ldb, ldc >= m); m == 0 or n == 0 returns
 * GEMMUL8_OK; on any error nothing is enqueued.  phase_ns as gemmul8_gemm.  gemmul8_work_size_trmm(side, m, n, N) ==
 * gemmul8_work_size(m, n, side == LEFT ? m : n, N, GEMMUL8_REAL_DEFAULT).
 * Complex form (ztrmm / ctrmm): type_a, type_b, type_c all in {C_64F, C_32F}, in the combinations gemmul8_gemm
 * accepts under a complex compute type; trans may also be GEMMUL8_OP_C (op(A) = A^H); alpha points to one complex
 * value of C's precision.  Neither part of an unreferenced element of A is read, a unit diagonal counts as 1 + 0i.
 * C carries the bits gemmul8_gemm writes for the dense form in fast mode under any complex compute type, in
 * accurate mode under GEMMUL8_COMPLEX_KARATSUBA_MULT (whose bound carries no reference defect).  The products
 * always run on the Karatsuba geometry: per modulus the three sub-products of the sub-blocks [re | im | re + im],
 * each tile of each over the k-steps the triangle leaves nonzero ("gemm_i8_trmm_kara_kernel" /
 * "gemm_i8_trmm_kara_onetile_kernel"), so a skipped k-step is skipped three times; padded k beyond 2^16 runs
 * gemmul8_gemm's products over all tiles of the same layout.  The workspace is
 * gemmul8_work_size_trmm_complex(side, m, n, N), the Karatsuba layout's size at every shape (==
 * gemmul8_work_size(m, n, side == LEFT ? m : n, N, GEMMUL8_COMPLEX_KARATSUBA_MULT) wherever gemmul8_gemm takes that
 * geometry). */
enum { GEMMUL8_SIDE_LEFT = 0, GEMMUL8_SIDE_RIGHT = 1 };
enum { GEMMUL8_DIAG_NON_UNIT = 0, GEMMUL8_DIAG_UNIT = 1 };
size_t gemmul8_work_size_trmm(int side, size_t m, size_t n, unsigned num_moduli);
size_t gemmul8_work_size_trmm_complex(int side, size_t m, size_t n, unsigned num_moduli);
int gemmul8_trmm(void *stream, int side, int uplo, int trans, int diag, size_t m, size_t n, int type_a, int type_b,
                 int type_c, const void *alpha, const void *A, size_t lda, const void *B, size_t ldb, void *C,
                 size_t ldc, unsigned num_moduli, int fastmode, void *work, double *phase_ns);

/* --- phase entry points (multi-GPU sharding, gemmul8/dist.py) ------------------------------------
 * gemmul8_gemm == gemmul8_split(0, N) + gemmul8_products(0, N) + gemmul8_recombine, on one stream.
 * Splitting the moduli range lets a rank produce only the residue planes [mod_begin, mod_end)
 * (plane j at work + offR + j * planeR, see gemmul8_layout), e.g. to send them to a root that runs
 * gemmul8_recombine (gemm_moduli_planes_to_root); the sharded entry points further below split the
 * columns too, and the CRT with them (gemm_moduli).
 *
 * Accurate mode couples the shifts of op(B)'s columns to every row of op(A) (the int8 bound
 * product's column maxima).  A row-block shard therefore runs gemmul8_split_bound, combines the
 * column maxima (int32 [n] at work + offBound + 4 * m_pad) with a MAX all-reduce, and calls
 * gemmul8_split with GEMMUL8_SPLIT_BOUND_READY.
 *
 * One workspace may serve several gemmul8_products / _products_cols launches in flight on
 * different streams only when their mod_begin differ (each first modulus has its own tile-queue
 * heads); launches ordered on one stream may share anything.
 *
 * The phase entry points never split k: gemmul8_products / _products_cols run one block per output tile and
 * modulus over the whole of k (in sequential chunks beyond padded k = 2^17) at every shape.  gemmul8_gemm runs
 * launches of few tiles and long k as "gemm_i8_splitk_kernel", whose residues are the same bytes. */
enum { GEMMUL8_SPLIT_BOUND_READY = 1, GEMMUL8_SPLIT_SHIFTS_READY = 2 };
int gemmul8_split_bound(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b,
                        int type_c, const void *A, size_t lda, const void *B, size_t ldb, unsigned num_moduli,
                        void *work, int compute_type);
/* flags: GEMMUL8_SPLIT_BOUND_READY (accurate: bound maxima in the workspace, derive the shifts from
 * them), GEMMUL8_SPLIT_SHIFTS_READY (sftA / sftB already in the workspace: encode the slices only).
 * mod_begin == mod_end: the shifts only, no slices (e.g. an accurate-mode shard that multiplies no
 * modulus but recombines columns). */
int gemmul8_split(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b, int type_c,
                  const void *A, size_t lda, const void *B, size_t ldb, unsigned num_moduli, int fastmode, void *work,
                  int compute_type, unsigned mod_begin, unsigned mod_end, int flags);
int gemmul8_products(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type, void *work,
                     unsigned mod_begin, unsigned mod_end);
int gemmul8_recombine(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int type_c, int compute_type,
                      const void *alpha, const void *beta, void *C, size_t ldc, void *work);

/* --- sharded entry points (the moduli x column-block partition of gemmul8/dist.py) ---------------
 * Every output element's CRT needs all N residues, and every residue plane is column-major
 * (plane j, column c at work + offR + j * planeR + c * ldr), so a column range of a plane is one
 * contiguous run of bytes.  A job over W ranks: (1) each rank computes the shifts of its own
 * rows / columns (gemmul8_shard_stats), the ranks all-gather the int16 shift vectors into every
 * workspace (offSftA / offSftB; accurate mode: sft0 at offSft0, A's rows then B's columns from
 * bm_pad), accurate mode then runs gemmul8_shard_bound over its column range and MAX-all-reduces
 * the bound area (int32 [bm_pad + n_pad] at offBound); (2) gemmul8_split(..., SHIFTS_READY or
 * BOUND_READY) encodes its moduli; (3) gemmul8_products_cols produces its (modulus, column-range)
 * units; (4) the ranks exchange the residue column runs so each holds all N planes of its own
 * output columns; (5) gemmul8_recombine_cols.  Row / column range starts are multiples of 256
 * (the product tile) for products_cols / shard_bound; range ends are multiples of 256 or n.
 * The result is bit-identical to gemmul8_gemm on the same operands. */
/* fast mode: sftA[row_begin, row_end) and sftB[col_begin, col_end); accurate mode: the sft0 of the same ranges */
int gemmul8_shard_stats(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b,
                        int type_c, const void *A, size_t lda, const void *B, size_t ldb, unsigned num_moduli,
                        int fastmode, void *work, int compute_type, size_t row_begin, size_t row_end,
                        size_t col_begin, size_t col_end);
/* accurate mode, sft0 assembled: magnitude planes + the bound product over columns [col_begin, col_end)
 * (the bound area is zeroed first; the other columns' maxima stay 0) */
int gemmul8_shard_bound(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b,
                        int type_c, const void *A, size_t lda, const void *B, size_t ldb, unsigned num_moduli,
                        void *work, int compute_type, size_t col_begin, size_t col_end);
/* residue planes [mod_begin, mod_end), columns [col_begin, col_end) only (one launch) */
int gemmul8_products_cols(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type,
                          void *work, unsigned mod_begin, unsigned mod_end, size_t col_begin, size_t col_end);
/* CRT + scaling + epilogue of the output columns [col_begin, col_end); C points at column col_begin */
int gemmul8_recombine_cols(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int type_c,
                           int compute_type, const void *alpha, const void *beta, void *C, size_t ldc, void *work,
                           size_t col_begin, size_t col_end);

/* --- partial CRT sums (the north star's "single RCCL reduce of partial FP64 accumulators") ------
 * A rank holding the residue planes of moduli [mod_begin, mod_end) (gemmul8_split + gemmul8_products of that
 * range, every shift in its workspace) writes per output element the partial CRT sums of its range into
 * sums = column-major double [2][n][lds] (plane 0: C1 = sum hi_i r_i, plane 1: C2 = sum lo_i r_i; one-level
 * moduli, N <= 7 or float output: C1 = sum NMi_i r_i, C2 = 0) -- inverse_scaling.hpp:35-62, 138-172
 * restricted to the range.  The element-wise sums of all ranks' planes (an RCCL sum reduce) finish into C with
 * gemmul8_crt_finish (sftA / sftB from `work`).  Not bit-identical to gemmul8_gemm; how close depends on the
 * moduli level:
 *   two-level (f64 output, N >= 8): C1 is exact in any order, only C2's rounded sum is reordered: C within a
 *     few ulp, max |C - C_gemm| <= 2^-40 max |C_gemm| in the tests;
 *   one-level, N <= 5 (f64): every partial sum stays below 2^53, so C1 is exact: the same few-ulp bound;
 *   one-level, N = 6, 7 (f64): C1 = sum NMi_i r_i exceeds 2^53 and is rounded in whatever order the reduce
 *     takes (the single call's own C carries an error of that size): max |C - C_gemm| <= 2^-26 max |C_gemm|;
 *   float output (one-level at every N): the same reordering, then the rounding to float:
 *     max |C - C_gemm| <= 2^-19 max |C_gemm|.
 * Real outputs only (GEMMUL8_E_UNSUPPORTED for complex compute types). */
int gemmul8_crt_partial(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int type_c,
                        int compute_type, const void *work, unsigned mod_begin, unsigned mod_end, double *sums,
                        size_t lds);
int gemmul8_crt_finish(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int type_c,
                       int compute_type, const void *alpha, const void *beta, void *C, size_t ldc, const void *work,
                       const double *sums, size_t lds);

/* --- instrumentation (used by bench.py / tests) --------------------------------------------- */
/* When enabled, every gemmul8_gemm records HIP events between its phases on its stream; the
 * accumulated per-phase milliseconds and the call count are read (and reset) with
 * gemmul8_timing_read, which synchronises on the recorded events. */
void gemmul8_timing_enable(int on);
int gemmul8_timing_read(double *phase_ms /* [4] */, int *calls);

/* Workspace layout for a shape: fills out[0..23] = {m_pad, n_pad, k_pad, ksteps, planeA, planeB,
 * planeR, offA, offB, offR, offSftA, offSftB, offBound, offSft0, total, kblk, ldr, nsub, subA, subB,
 * subR, vsA, vsB, bm_pad}.  Complex compute types run Karatsuba products: per modulus the slice planes
 * hold the sub-blocks [re | im | re + im] (vsA rows / vsB columns each, subA / subB bytes apart) and the
 * residue plane the three products Ar Br, Ai Bi, (Ar + Ai)(Br + Bi) (subR bytes apart, ld = ldr);
 * nsub = 1 otherwise.  The accurate-mode bound maxima are rows [0, bm_pad) then columns. */
int gemmul8_layout(size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type, size_t *out);

/* Validation hook: int32 product of plane 0 of the tiled int8 operands already in `work`
 * (layout of gemmul8_layout) into C32 (column-major, ld = m_pad).  Used by the MFMA tests. */
int gemmul8_i8_product_raw(void *stream, size_t m, size_t n, size_t k, unsigned num_moduli, int compute_type,
                           void *work, int32_t *C32);

/* Validation hook: exhaustive exactness check of the product kernel's residue epilogue against exact
 * arithmetic, for all 20 moduli -- path 0: the biased reduction (integer Barrett) over every x in
 * [-2^30, 2^30]; path 3: the same range through the f64 form the product kernels use; path 1: the
 * reference's signed Barrett step (conv_32i_2_8u.hpp:7-56) over every int32.  Returns the number of
 * mismatching (input, modulus) pairs (0 expected; path 2 is a negative control that compares path 0
 * with a wrong expectation, so every pair mismatches). */
unsigned long long gemmul8_residue_selftest(void *stream, int path);

/* Epilogue semantics of C = alpha * AB + beta * C, process-wide (default GEMMUL8_EPILOGUE_BLAS; the
 * environment variable GEMMUL8_EPILOGUE=reference selects the other at load time).
 *   GEMMUL8_EPILOGUE_BLAS       BLAS: beta = 0 never reads C; alpha = 1 with another beta is
 *                               beta * C + AB; beta = 1 is alpha * AB + C at every moduli count.
 *   GEMMUL8_EPILOGUE_REFERENCE  the reference's kernels bit for bit, its non-BLAS variants included
 *                               (inverse_scaling.hpp): alpha = 1 with beta off {0, 1} computes beta * AB + C
 *                               (_1b, :417, :682), alpha != 1 with beta = 1 at num_moduli >= 8 (two-level
 *                               moduli, real and complex double output) computes alpha * C + AB (_2_a1,
 *                               :736, :763), and alpha != 1 with beta = 0 reads C as fma(0, C, alpha * AB)
 *                               (_ab, :522, :549, :791, :819: NaN / Inf in C propagate).
 * Returns GEMMUL8_E_UNSUPPORTED for an unknown mode.  Takes effect for calls enqueued afterwards. */
enum { GEMMUL8_EPILOGUE_BLAS = 0, GEMMUL8_EPILOGUE_REFERENCE = 1 };
int gemmul8_set_epilogue(int mode);
int gemmul8_get_epilogue(void);

/* Name of the residue-product kernel the last products launch of this process took
 * ("gemm_i8_persistent_pg_kernel", "gemm_i8_persistent_kernel", "gemm_i8_kernel", "gemm_i8_small_kernel",
 * "gemm_i8_kernel (k-chunked)", "gemm_i8_batched_kernel", "gemm_i8_batched_onetile_kernel", "gemm_i8_syrk_kernel",
 * "gemm_i8_syrk_onetile_kernel", "gemm_i8_herk_kernel", "gemm_i8_herk_onetile_kernel", "gemm_i8_trmm_kernel",
 * "gemm_i8_trmm_onetile_kernel", "gemm_i8_trmm_kara_kernel", "gemm_i8_trmm_kara_onetile_kernel" (complex
 * gemmul8_trmm), "gemm_i8_splitk_kernel" (gemmul8_gemm and its low-memory, strided-batched-fallback
 * and timing forms only: few output tiles, long k) or "none"; a gemmul8_syrk, gemmul8_herk or gemmul8_trmm call outside its own
 * kernels' domain reports the gemm kernel that ran all tiles). */
const char *gemmul8_last_products_kernel(void);

/* --- bench / test harness (not part of the emulation path) ------------------------------------ */
/* The reference's input generator (testing/make_matrix.hpp:8-71): x = (U(0,1] - 0.5) * exp(phi * N(0,1))
 * from hiprand XORWOW, init(seed, idx, 0); complex draws (u_re, n_re, u_im, n_im). dtype: GEMMUL8_*. */
int gemmul8_randmat(void *stream, int dtype, size_t m, size_t n, void *A, double phi, unsigned long long seed);
/* Double-double reference product C1 + C2 = A * B (testing/eval.hpp:265-308); A m x k, B k x n, col-major. */
int gemmul8_dd_gemm(void *stream, size_t m, size_t n, size_t k, const double *A, const double *B, double *C1,
                    double *C2);
/* err[i] = |C[i] - (C1[i] + C2[i])| / |C1[i] + C2[i]| evaluated in double-double (eval.hpp:317-338). */
int gemmul8_relerr_dd(void *stream, size_t count, const double *C, const double *C1, const double *C2, double *err);
/* the reference drivers' timing loop (GEMMul8/testing/test_double.cu:422-431) in native code: `iters` calls of
 * gemmul8_gemm, each bracketed by hipDeviceSynchronize and the host clock; *sec = mean seconds per call (calls
 * without phase events), phase_ns[4] = mean phase times from a second loop of `iters` calls (NULL: not run) */
int gemmul8_time_gemm(void *stream, int op_a, int op_b, size_t m, size_t n, size_t k, int type_a, int type_b,
                      int type_c, const void *alpha, const void *A, size_t lda, const void *B, size_t ldb,
                      const void *beta, void *C, size_t ldc, unsigned num_moduli, int fastmode, void *work,
                      int compute_type, int iters, double *sec, double *phase_ns);
/* the same loop around the vendor GEMM of the drivers (test_double.cu:318-331): hipblasGemmEx op N / N, alpha 1,
 * beta 0, every operand of `type`, lda = m, ldb = k, ldc = m */
int gemmul8_time_vendor_gemm(void *stream, int type, size_t m, size_t n, size_t k, const void *A, const void *B,
                             void *C, int iters, double *sec);
/* Data-bound ceiling of the int8 products: TOPS of the better of v_mfma_i32_32x32x32_i8 and
 * v_mfma_i32_16x16x64_i8 alone on uniformly random operand bytes held in registers (2 waves per
 * SIMD, the ops of `iters` x 64 32x32x32 MFMAs per wave); synchronises. */
double gemmul8_mfma_ceiling(void *stream, int iters);

#ifdef __cplusplus
}
#endif
#endif /* GEMMUL8_C_H */
