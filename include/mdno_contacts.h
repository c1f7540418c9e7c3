/*
 * mdno_contacts.h — sixteenth public header of libmdno.so: contact statistics of a trajectory that already lies in device
 * memory (csrc/contacts.hip) — per pair and time block the number of frames in contact and the sums of the
 * distance and of its square (contact-probability maps, mean-distance maps), the contact indicator of a list of pairs as
 * one bit per step (the fraction of native contacts Q(t)), and from those bits the contact autocorrelation at a set of
 * lags (how long a contact lives).  Additive, like mdno_observe.h: include/mdno.h, include/mdno_train.h and their version
 * numbers stay as they are, and no launch, captured graph or bit of an existing entry point changes.  (This file is part
 * of the library's content hash, and csrc/contacts.hip includes it, so a declaration that drifts from its definition does
 * not compile; tests/test_cabi_tables.py holds it to the ctypes table and the exports.)  Conventions as in mdno.h: device
 * pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as void*, 0 or a negative MDNO_E* code
 * (mdno_last_error() has the message), every refusal before any device work.  The entry points are named mdnocm_*.
 *
 * THE RULE.  frames is f32 [S, M, N, 3] (step, member, atom: the rollout engine's own layout).  box is NULL or HOST
 * f64 [3] as in mdno_pbc.h (0 = open axis; every periodic axis needs L >= 2 * cut, cut = threshold or cut_max below, so a
 * pair has one image inside the cut; an all-open box is the same as NULL).  For atoms i, j of ONE frame, all in fp64 on
 * the fp32 coordinates, no FMA contraction:
 *     d_a = (double)x_j[a] - (double)x_i[a]            reduced on a periodic axis as in mdno_pbc.h:
 *                                                      d_a -= rint(d_a * invL) * L, invL = 1.0 / L formed on the host
 *     s   = (dx*dx + dy*dy) + dz*dz,   r = sqrt(s)     (the summation order and the root of the radius graph's test)
 *     the pair is IN CONTACT iff r < cut               (strict; a NaN or an Inf anywhere makes the comparison false)
 * The rule is symmetric in i and j bit for bit (the differences change sign, rint is odd, the squares do not change).  It
 * applies to i == j as well: r = 0 there, so a finite atom is in contact with itself, as in mdno_contact_maps; an atom
 * with a NaN or Inf coordinate is not (Inf - Inf = NaN).  Frames are never wrapped: atoms many box lengths apart are
 * reduced by the rint above.
 * (sqrt is correctly rounded and so monotone: where only the indicator is asked, a kernel may test s < s*, with s* the
 * smallest double whose root is >= cut, found on the host.  It is the same set of pairs.)
 *
 * (a) PAIR STATISTICS OVER TIME BLOCKS (mdnocm_pair_statistics).  Step s belongs to block s / block_len, block_len >= 1,
 * Bk = ceil(S / block_len) blocks (the last may be short).  Three outputs, each [Bk, M, N, N] row-major, FULL symmetric
 * maps (both triangles and the diagonal are written, out[b, m, i, j] and out[b, m, j, i] hold the same bits):
 *     count  i32   the frames of the block in which (i, j) is in contact at cut = threshold
 *     sum_r  f64   acc = acc + r  over the frames of the block, in ASCENDING step order, starting from 0.0
 *     sum_r2 f64   acc = acc + s  likewise
 * One sequential chain per pair and sum: a block's bits depend on its frames, the threshold and the box alone — not on S, M,
 * the other members, the tile or the run.  Non-finite values propagate into the sums (a NaN marks the pair) and are not
 * counted.  sum_r or sum_r2 may be NULL: that sum is neither computed nor stored.  No floating-point atomics, no atomics
 * at all; every element of the outputs is stored exactly once.  Element indices are 64-bit.
 *
 * (b) CONTACT SERIES OF A PAIR LIST (mdnocm_contact_bits).  pairs i32 [P, 2] and cut f64 [P] on the device, one cutoff per
 * pair; cut_max HOST f64, finite and > 0, is what the box is checked against.  Pair p is in contact at step s of member m
 * iff r < cut[p] AND r < cut_max (both strict; a NaN cut is never in contact).  An index outside 0 .. N - 1 gives "not in
 * contact" and reads nothing.  Repeated pairs and i == j are pairs like any other.
 *     bits      u64 [M, P, Wd], Wd = ceil(S / 64): bit s % 64 of word s / 64 of row (m, p) is the indicator at step s;
 *               the bits from S on are 0.  Every word is stored exactly once.
 *     per_frame i32 [S, M]: how many of the P listed pairs are in contact in that frame (the numerator of Q(t)): zeroed
 *               on the stream, then added to with integer atomics — exact in any order.
 *
 * (c) CONTACT CORRELATION (mdnocm_contact_correlation).  bits as (b) wrote them (bits from S on are never looked at), lags HOST
 * i32 [L], every lag in 0 .. S - 1, L in 0 .. MDNOCM_MAX_LAGS.  With c(t) the indicator of (m, p) at step t:
 *     origins[m, p, l] = #{t in [0, S - lag) : c(t)}
 *     both[m, p, l]    = #{t in [0, S - lag) : c(t) and c(t + lag)}
 * both i32 [M, P, L]: shifted words, AND, population count.  Integers, exact.
 */
#ifndef MDNO_CONTACTS_H
#define MDNO_CONTACTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDNOCM_TILE 64            /* atoms per side of a pair tile of mdnocm_pair_statistics */
#define MDNOCM_PAIR_CHUNK 256     /* listed pairs per workgroup of mdnocm_contact_bits */
#define MDNOCM_MAX_LAGS 1024

/* frames f32 [S, M, N, 3] -> count i32, sum_r f64, sum_r2 f64 [ceil(S / block_len), M, N, N] by (a) above.  One workgroup
 * of 256 threads owns a MDNOCM_TILE x MDNOCM_TILE tile of pairs of one (block, member) with tile row <= tile column, keeps
 * the accumulators of its 16 pairs per thread in registers, walks the block's frames in step order with the two tiles'
 * coordinates staged in LDS (the next frame is loaded while this one is worked on) and stores its tile and its mirror.
 * MDNO_EINVAL before any device work for S, M or N < 0, block_len < 1, threshold not finite or <= 0, a bad box (the
 * messages of mdno_pbc.h), a null frames or count where they are needed; MDNO_EUNSUPPORTED for M or the number of blocks
 * above 65,535 or more than 2^31 - 1 tiles of one map (the launch grid).  S == 0, M == 0 or N == 0: returns 0, touches
 * nothing. */
int mdnocm_pair_statistics(const float* frames, int S, int M, int N, double threshold, const double* box, int block_len,
                           int32_t* count, double* sum_r, double* sum_r2, void* stream);

/* frames f32 [S, M, N, 3], pairs i32 [P, 2], cut f64 [P] -> bits u64 [M, P, ceil(S / 64)], per_frame i32 [S, M] by (b)
 * above.  A wave takes 64 consecutive steps of one pair, one step per lane, and forms the word with the wave-wide ballot; a
 * workgroup owns MDNOCM_PAIR_CHUNK pairs of one (word, member) and adds its per-step counts to per_frame once.  per_frame
 * may be NULL (not formed).  MDNO_EINVAL before any device work for a negative size, cut_max not finite or <= 0, a bad box,
 * a null pointer where one is needed; MDNO_EUNSUPPORTED for M or the number of words above 65,535.  S == 0, M == 0 or
 * P == 0: returns 0, touches nothing. */
int mdnocm_contact_bits(const float* frames, int S, int M, int N, const int32_t* pairs, const double* cut, int P,
                        double cut_max, const double* box, uint64_t* bits, int32_t* per_frame, void* stream);

/* bits u64 [M, P, ceil(S / 64)], lags HOST i32 [L] -> origins, both i32 [M, P, L] by (c) above: one thread per
 * (member, pair, lag).  MDNO_EINVAL before any device work for a negative size, L > MDNOCM_MAX_LAGS, a lag outside
 * 0 .. S - 1, a null pointer where one is needed.  S == 0, M == 0, P == 0 or L == 0: returns 0, touches nothing. */
int mdnocm_contact_correlation(const uint64_t* bits, int S, int M, int P, const int32_t* lags, int L, int32_t* origins,
                               int32_t* both, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_CONTACTS_H */
