/*
 * mdno_internal.h — twelfth public header of libmdno.so: internal coordinates of frames that already lie in device memory
 * (csrc/internal.hip) — selected pair distances, bond angles (as their cosine) and dihedrals (as cosine and
 * sine) per frame, written as the rows of a feature matrix that mdnopca_* and mdnomsm_* take as they are; and a per-column
 * histogram of such a matrix.  These features do not depend on a reference frame: a rigid rotation or translation of a
 * frame changes them by rounding only.  Additive, like mdno_markov.h: include/mdno.h, include/mdno_train.h and their
 * version numbers stay as they are, and no launch, captured graph or bit of an existing entry point changes.  (This file
 * is part of the library's content hash, and csrc/internal.hip includes it, so a declaration that drifts from its
 * definition does not compile; tests/test_cabi_tables.py holds it to the ctypes table and the exports.)  Conventions
 * as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*, 0 or a negative
 * MDNO_E* code (mdno_last_error() has the message), every refusal before any device work.
 *
 * THE PREFIX.  The entry points are named mdnoic_*, not mdno_*.  The prefix is kept because the names are ABI;
 * nothing else asks for it (names need only be unique over all headers, which tests/test_cabi_tables.py checks).
 * The functions live in the same library, under the same content hash and the same
 * mdno_abi_version().
 *
 * FEATURES (mdnoic_features).  frames f32 [F, N, 3]; index arrays i32 on the device: pairs [P, 2], triples [A, 3],
 * quads [T, 4] (null where the count is 0); box NULL or HOST f64 [3], 0 = open axis (mdno_pbc.h); out [F, D] row-major of
 * `out_dtype`, D = P + A + 2 T: the P distances, the A angle cosines, then (cos, sin) of dihedral 0, (cos, sin) of
 * dihedral 1, ...  With MDNO_IC_RADIANS in `flags` an angle is one column in radians and so is a dihedral: D = P + A + T.
 *
 * THE RULE.  fp64 on the fp32 coordinates; the operations + - x / sqrt rint only, each rounded once (no FMA contraction),
 * in exactly this order.  x_a[c] is component c of atom a of the frame.
 *   bond vector   v(a->b)_c = (double)x_b[c] - (double)x_a[c];   on a periodic axis (L_c > 0), with invL_c = 1.0 / L_c
 *                 formed on the host:  v_c = v_c - rint(v_c * invL_c) * L_c   (rint: to nearest, ties to even).  No cutoff
 *                 is tested: the caller owns the validity of the minimum image.  An open axis leaves v_c as it is.
 *   dot product   p . q = (p_x q_x + p_y q_y) + p_z q_z
 *   cross product (p x q)_x = p_y q_z - p_z q_y,  (p x q)_y = p_z q_x - p_x q_z,  (p x q)_z = p_x q_y - p_y q_x
 *                 (two rounded products and one subtraction per component)
 *   clamp(c)      c > 1 ? 1 : (c < -1 ? -1 : c)        — a NaN fails both tests and passes through
 *   distance  of (i, j):        v = v(i->j);  r = sqrt(v . v)
 *   angle     of (i, j, k), at the middle atom j:  u = v(j->i), w = v(j->k);
 *                 c = (u . w) / (sqrt(u . u) * sqrt(w . w));  feature clamp(c).  A zero-length bond gives 0 / 0 = NaN.
 *   dihedral  of (i, j, k, l), IUPAC sign (looking along j->k, the clockwise rotation that carries i onto l is positive):
 *                 b1 = v(i->j), b2 = v(j->k), b3 = v(k->l);  n1 = b1 x b2,  n2 = b2 x b3;
 *                 x = n1 . n2;  y = sqrt(b2 . b2) * (b1 . n2);  h = sqrt(x * x + y * y);
 *                 features clamp(x / h), clamp(y / h).  Collinear atoms give h = 0, hence NaN in both columns: j, k, l on a
 *                 line (b3 an exact multiple of b2, or zero) make n2 = 0 exactly, so x = y = 0; i, j, k on a line make
 *                 n1 = 0 and x = 0, and y = 0 wherever b1 . n2 is formed without rounding (otherwise what rounding leaves
 *                 of it decides: next to a collinear triple a dihedral is ill-conditioned, and a small h says so).
 *   MDNO_IC_RADIANS: angle = acos(clamp(c)); dihedral = atan2(y, x) where h > 0, NaN otherwise (h is 0 or NaN).  acos and
 *                 atan2 are the device math library's: not correctly rounded, a few ulp (README has the measured figure);
 *                 everything before them is the rule above, bit for bit.
 *   AN INDEX outside 0 .. N - 1 makes that feature NaN (both columns of a dihedral).  The kernel tests the index and reads
 *   nothing for that feature: no read outside the frame, no status word, no read-back.
 *   NON-FINITE COORDINATES propagate through the arithmetic to the features that touch them and to no others.
 *   f32 OUTPUT is the fp64 value rounded once (to nearest even).
 *   The bits of a feature depend on its frame, its index tuple, the box and the flags alone — not on F, D, where the tuple
 *   stands in its array, the form or the run.  Nothing is summed across threads; there are no atomics.
 *
 * FORMS.  MDNO_IC_FORM_LDS (N <= MDNO_IC_LDS_ATOMS): a workgroup of MDNO_IC_WORKGROUP threads copies
 * MDNO_IC_FRAMES_PER_GROUP(N) consecutive whole frames into LDS as they lie in memory (fp32, 12 bytes per atom), then its
 * threads walk (frame, feature) of its MDNO_IC_FEATURE_CHUNK columns in strides of the workgroup, consecutive lanes on
 * consecutive columns: the index tuples are read coalesced, the coordinates gathered from LDS, out[f, d] stored
 * coalesced.  MDNO_IC_FORM_GLOBAL (any N): the same walk with the coordinates gathered from global memory.
 * MDNO_IC_FORM_AUTO: LDS where N allows it.  The arithmetic is one function that both forms call.
 *
 * COLUMN HISTOGRAM (mdnoic_column_histogram).  x [R, D] of `dtype`; lo, hi HOST f64 [D], or [1] shared by all columns when
 * `shared_range` is non-zero; counts i64 [D, n_bins + 2], n_nan i64 [D].  (`groups` = G > 1: x is [R, G D], G groups of D
 * columns that share the D ranges — the members of a feature tensor [S, M, D] —, counts [G D, n_bins + 2], n_nan [G D].)
 * Per column a, with
 * inv_w_a = (double)n_bins / (hi_a - lo_a) formed on the host and v = (double)x_ra:
 *     v is NaN                       -> n_nan[a] += 1, no bin
 *     v < lo_a                       -> bin 0                      ("below lo")
 *     v >= hi_a                      -> bin n_bins + 1             ("at or above hi")
 *     otherwise b = (long long)((v - lo_a) * inv_w_a), b == n_bins -> n_bins - 1 (the rounding case of mdno_observe.h),
 *                                       bin b + 1
 *   so counts[a].sum() + n_nan[a] == R.  Integer atomics only: a private table per workgroup in LDS (u32; a workgroup
 *   counts at most MDNO_IC_HIST_ROWS rows), flushed into counts with 64-bit integer adds; counts are exact in any order.
 *   The ranges travel by value in the kernel arguments, MDNO_IC_HIST_COLUMNS columns per launch.
 */
#ifndef MDNO_INTERNAL_H
#define MDNO_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types of `out` and of a histogram's x */
#define MDNO_IC_F32 0
#define MDNO_IC_F64 1
/* flags of mdnoic_features */
#define MDNO_IC_RADIANS 1
/* forms */
#define MDNO_IC_FORM_AUTO 0
#define MDNO_IC_FORM_LDS 1
#define MDNO_IC_FORM_GLOBAL 2
/* threads of a workgroup; the largest N of the LDS form (24 KiB of fp32 coordinates per workgroup); the most frames a
 * workgroup stages; the columns of a frame one workgroup owns */
#define MDNO_IC_WORKGROUP 256
#define MDNO_IC_LDS_ATOMS 2048
#define MDNO_IC_MAX_GROUP_FRAMES 16
#define MDNO_IC_FEATURE_CHUNK 8192
/* frames per workgroup (both forms): as many whole frames as MDNO_IC_LDS_ATOMS atoms hold, 1 .. MDNO_IC_MAX_GROUP_FRAMES */
#define MDNO_IC_FRAMES_PER_GROUP(N)                                                              \
    ((N) <= 0 || MDNO_IC_LDS_ATOMS / (N) < 1 ? 1                                                 \
     : MDNO_IC_LDS_ATOMS / (N) > MDNO_IC_MAX_GROUP_FRAMES ? MDNO_IC_MAX_GROUP_FRAMES             \
                                                          : MDNO_IC_LDS_ATOMS / (N))
/* column histogram: the most bins; rows per workgroup; counters of a workgroup's LDS table; columns per launch */
#define MDNO_IC_MAX_BINS 4096
#define MDNO_IC_HIST_ROWS 4096
#define MDNO_IC_HIST_TABLE 8192
#define MDNO_IC_HIST_COLUMNS 128

/* frames f32 [F, N, 3], pairs i32 [P, 2], triples i32 [A, 3], quads i32 [T, 4] (device), box NULL or HOST f64 [3] ->
 * out [F, D] of out_dtype.  MDNO_EINVAL for negative sizes, an out_dtype, a form or flags other than the above,
 * MDNO_IC_FORM_LDS with N > MDNO_IC_LDS_ATOMS, a box entry that is negative or not finite, D beyond 2^31 - 1, a null index
 * array whose count is > 0, a null frames with F N > 0 (and D > 0), a null out with F D > 0; MDNO_EUNSUPPORTED where F
 * exceeds the launch grid.  F == 0 or D == 0: returns 0 and touches nothing. */
int mdnoic_features(const float* frames, int64_t F, int N, const int32_t* pairs, int P, const int32_t* triples, int A,
                    const int32_t* quads, int T, const double* box, int flags, int out_dtype, void* out, int form,
                    void* stream);

/* x [R, groups D] of dtype (device), lo and hi HOST f64 [D] ([1] with shared_range) -> counts i64 [groups D, n_bins + 2],
 * n_nan i64 [groups D]; groups = 1 is the plain matrix.  MDNO_EINVAL for negative sizes, groups D beyond 2^31 - 1, a bad
 * dtype, n_bins outside 1 .. MDNO_IC_MAX_BINS, a null lo or hi, a range that is not finite or has hi <= lo, a null counts or
 * n_nan, a null x with R > 0; MDNO_EUNSUPPORTED where R or groups (> 65535) exceeds the launch grid.  D == 0 or
 * groups == 0: returns 0 and touches nothing.  R == 0: zeros. */
int mdnoic_column_histogram(const void* x, int64_t R, int D, int groups, int dtype, const double* lo, const double* hi,
                            int shared_range, int n_bins, int64_t* counts, int64_t* n_nan, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_INTERNAL_H */
