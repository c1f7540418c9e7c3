/*
 * mdno_noise.h — third public header of libmdno.so: seeded Gaussian noise on the device (csrc/philox.h,
 * csrc/noise.hip).  Additive: include/mdno.h, include/mdno_train.h and their version numbers stay
 * as they are.  (A header of its own, like mdno_train.h, because the set of entry points of mdno.h that write caller
 * memory is pinned, name by name, by that header's guard-band table in tests/test_gpu_bounds.py; these three have
 * their table in tests/test_gpu_noise.py.  This file is part of the library's content hash, as every header
 * under include/ is, and csrc/noise.hip and csrc/engine.hip include it, so a declaration that drifts from its definition
 * does not compile; tests/test_cabi_tables.py holds it to the ctypes table and the exports.)
 * Conventions as in mdno.h: device pointers owned by the caller, explicit sizes, `stream` a hipStream_t passed as
 * void*, 0 or a negative MDNO_E* code (mdno_last_error() has the message).
 *
 * The generator is Philox4x32-10 with key = the 64-bit seed and counter
 *     (stream_id, index & 0xffffffff, element >> 2, purpose | second << 8 | (index >> 32) << 16),
 * word (element & 3) of the block; u = ((w >> 8) + 0.5f) * 2^-24 from the block with second = 0 (u1) and with
 * second = 1 (u2); z = sqrtf(-2 logf(u1)) * cosf(6.2831853f * u2).  0 <= index < 2^48, 0 <= purpose < 256.
 * A value depends on (seed, stream_id, index, element, purpose) alone: not on the launch, the batch, the rank,
 * graph replay or what is drawn beside it.  No atomics: two calls give the same bits.
 */
#ifndef MDNO_NOISE_H
#define MDNO_NOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDNO_NOISE_ROLLOUT 0      /* stream_id = global member, index = absolute step, element = atom * 3 + c */
#define MDNO_NOISE_TRAIN_WINDOW 1 /* stream_id = sample index in its dataset, index = epoch,
                                     element = (frame_in_window * N + atom) * 3 + c */

typedef struct mdno_rollout_plan mdno_rollout_plan;

/* The raw generator: z_out f32 [M, per_stream_elems] = sigma * z for streams stream_ids i32 [M] (device) and
 * elements 0 .. per_stream_elems - 1; per_stream_elems must be a multiple of 3 * N (N atoms: one frame of a
 * rollout, a whole window in training).  words_out u32 [M, per_stream_elems, 2], or NULL: the two Philox words
 * every element was made from ([..][0] gives u1, [..][1] u2). */
int mdno_noise_fill(uint64_t seed, const int32_t* stream_ids, int M, int64_t index, int N, int per_stream_elems,
                    int purpose, float sigma, float* z_out, uint32_t* words_out, void* stream);

/* Noise on the input windows of a collated training batch: x_out = x_in + sigma * z over x f32 [W, R, 3]
 * (time-major; x_out may be x_in).  Sample b owns rows row_offsets[b] .. row_offsets[b + 1] - 1 (i32 [B + 1],
 * device, ascending from 0 to R; at most max_rows_per_sample rows each) and draws from stream sample_ids[b]
 * (i32 [B], device: its index in the dataset) at index `epoch`, purpose MDNO_NOISE_TRAIN_WINDOW.  Targets, edge
 * attributes and the edge list are not touched. */
int mdno_noise_add_window(uint64_t seed, const int32_t* sample_ids, const int32_t* row_offsets, int B, int W,
                          int64_t R, int max_rows_per_sample, int64_t epoch, float sigma, const float* x_in,
                          float* x_out, void* stream);

/* Stochastic rollout: from the next mdno_rollout_plan_run on, every step adds sigma * z(seed, member_ids[m],
 * absolute step, atom, component) to the frame it produces before anything else reads it — the stored frame,
 * the next windows and the next radius graph all see the noisy frame.  member_ids i32 [M] (device) must stay
 * valid as long as the plan.  Valid before the first mdno_rollout_plan_run after the plan was created (or its
 * trajectory reset); a plan created with use_graph re-captures its steps on the stream it was created with.
 * sigma = 0 restores the plain step: the launch sequence and the captured graph of a plan that never had noise. */
int mdno_rollout_plan_set_noise(mdno_rollout_plan* plan, float sigma, uint64_t seed, const int32_t* member_ids);

#ifdef __cplusplus
}
#endif
#endif /* MDNO_NOISE_H */
