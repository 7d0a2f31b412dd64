/*
 * egc_optim.h -- C ABI of the optimizer step of libegc_hip.so (gfx950): the second public header of the library.
 *
 * Every config of the reference trains with Adam(model.parameters(), lr, weight_decay=wd) under a ReduceLROnPlateau
 * (experiments/zinc/configs.py, mol/configs.py, cifar/configs.py, code/configs.py, exp_config.py).  egc_adam_step_f32
 * runs that step for ALL tensors of a parameter group as one launch.  The header stands alone (it includes nothing of
 * egc_hip.h) and is written in the subset egc_amd/_abi.py reads; egc_amd/_optim.py binds it.  The conventions are those of
 * egc_hip.h: device pointers unless stated otherwise, float32, nothing here allocates, frees or synchronises, every
 * launch goes to the caller's stream and records into a hipGraph, and the int results are egc_status values
 * (0 = EGC_OK, 1 = EGC_ERR_INVALID, 3 = EGC_ERR_HIP; egc_last_error() of egc_hip.h has the message).
 */
#ifndef EGC_OPTIM_H
#define EGC_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* egc_stream_t; /* a hipStream_t (as in egc_hip.h) */

/* Tensors of one launch: their descriptors travel BY VALUE in the kernel arguments (32 bytes each, 4 KB in all), so a
 * recording holds the addresses it was made with and nothing is uploaded.  More tensors take further launches. */
#define EGC_ADAM_MAX_TENSORS 120
/* Elements of a tensor that one workgroup updates (256 threads, one 16-byte access per array and thread). */
#define EGC_ADAM_BLOCK_ELEMS 1024

/* One tensor of a step (a HOST struct).  The tensor's first-moment and second-moment slices are
 * exp_avg[state_offset .. + numel) and exp_avg_sq[state_offset .. + numel); state_offset is a multiple of 4 elements
 * (16 bytes).  Workgroup w of the tensor (w < max(1, ceil(numel / EGC_ADAM_BLOCK_ELEMS))) keeps the tensor's step
 * count in steps[step_offset + w]: all copies are equal, steps[step_offset] is "the" counter.  (One word per workgroup,
 * not per tensor: a workgroup that read a shared word after another had bumped it would take the wrong step, and
 * ordering them takes an atomic.)  p and g may be aligned to 4 bytes only (a view): the kernel then uses 4-byte
 * accesses for that tensor. */
typedef struct {
  float* p;              /* [numel] the parameter, updated in place */
  float* g;              /* [numel] its gradient; zeroed after it is read if zero_grads */
  uint32_t state_offset;
  uint32_t step_offset;
  int64_t numel;         /* 0 <= numel < 2^31 (a tensor without elements still counts its step) */
} egc_adam_tensor;

int32_t egc_adam_max_tensors(void);          /* EGC_ADAM_MAX_TENSORS */
int64_t egc_adam_launches(int64_t n_tensors); /* launches egc_adam_step_f32 issues for n_tensors; 0 for n_tensors <= 0 */
int64_t egc_adam_launch_count(void);          /* launches issued by this process so far (tests and tools count with it) */

/* HOST function.  For tensors of numels[0 .. n_tensors) elements laid out back to back:
 *   blocks_out[k]         workgroups of tensor k: max(1, ceil(numels[k] / EGC_ADAM_BLOCK_ELEMS));
 *   state_offsets_out[k]  its offset into the state buffers, in elements: the running sum of the numels each rounded up to a
 *                         multiple of 4 (16 bytes).
 * Returns the length of a state buffer in elements (the last offset + the last rounded numel), or -1 for a null pointer,
 * a negative count, a numel outside [0, 2^31) or a total of 2^32 elements or more (offsets are 32-bit in the launch).
 * The step offsets of egc_adam_tensor are the running sum of blocks_out, its total the length of `steps`. */
int64_t egc_adam_plan(const int64_t* numels, int64_t n_tensors, int32_t* blocks_out, int64_t* state_offsets_out);

/* torch.optim.Adam's step (not AdamW: weight decay is L2 added to the gradient; no amsgrad, no maximize) for
 * tensors[0 .. n_tensors) (HOST array), egc_adam_launches(n_tensors) launches of one kernel:
 *     g' = g + weight_decay * p          (skipped when weight_decay == 0)
 *     m  = beta1 * m + (1 - beta1) * g'
 *     v  = beta2 * v + (1 - beta2) * (g' * g')
 *     t  = steps[..] + 1
 *     p  = p - (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 * Element arithmetic in float32 in exactly this order, IEEE sqrt and division, no contraction.  The three per-step factors
 * lr / (1 - beta1^t), sqrt(1 - beta2^t) and 1 - beta1 / 1 - beta2 are computed in float64 (the first two on the device from
 * the integer t and *lr_dev, once per workgroup) and rounded once.  lr_dev is a DEVICE double read by the kernel: a scheduler
 * that writes it changes the rate of a recorded step without a new recording.  No atomics; every word has one writer.
 * Returns EGC_ERR_INVALID before any launch for a null pointer (p, g of a tensor with elements included), a negative count,
 * a numel outside [0, 2^31), a state_offset that is no multiple of 4, p / g not aligned to 4 bytes or exp_avg / exp_avg_sq
 * not aligned to 16. */
int egc_adam_step_f32(const egc_adam_tensor* tensors, int64_t n_tensors, float* exp_avg, float* exp_avg_sq, int32_t* steps,
                      const double* lr_dev, double beta1, double beta2, double eps, double weight_decay, int32_t zero_grads,
                      egc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
