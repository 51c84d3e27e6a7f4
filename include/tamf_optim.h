/*
 * tamf_optim.h - C-ABI of the optimiser step (libtamf_optim.so): per-parameter gradient clipping followed by AdamW, over a table of
 * tensors, in two launches per step whatever the number of tensors.  It is what the reference runs after every backward as
 * util/net_util.py:clip_gradient (one clip_grad_norm_(param, 0.1, 2.0) per parameter) and torch.optim.AdamW.step().
 *
 * Arithmetic: torch's single-tensor path, per tensor, in float32 (t = step_index, the bias corrections are formed on the host in
 * double and rounded once):
 *     n  = sqrt(sum g^2);  c = min(1, max_norm / (n + 1e-6));  g' = c g          (no clipping: g' = g)
 *     p <- p (1 - lr wd);  m <- m + (g' - m)(1 - beta1);  v <- beta2 v + (1 - beta2) g'^2
 *     p <- p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * A NaN norm gives a NaN c (torch.clamp keeps NaN), so one NaN gradient element turns the whole tensor's p, m and v to NaN and
 * touches no other tensor.  The gradient is READ, never written: the reference scales it in place and then zeroes it.
 *
 * Layout: every tensor is contiguous float32 device memory owned by the caller, all on the context's device.  A tensor whose four
 * base addresses are 16-byte aligned is streamed with 16-byte accesses, any other with 4-byte accesses; both give the same bits.
 *
 * Determinism: no atomics, one writer per element, every sum in a fixed order that depends on the tensor's numel only.  The same
 * call gives the same bits, and a tensor's result does not depend on which other tensors share the table or where it stands in it.
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Every function returns 0 or a negative tamf_status; the
 * message of the calling thread's last failure is tamf_optim_last_error().  `stream` is a hipStream_t passed as void*.
 * tamf_optim_bind synchronises the device (the table it replaces may still be read); grad_norms and step synchronise nothing and
 * copy nothing to the host.
 */
#ifndef TAMF_OPTIM_H
#define TAMF_OPTIM_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TAMF_OPTIM_CHUNK 4096 /* elements of a tensor that one workgroup sums / updates */

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_optim_last_error(void);

/* a context on `device` (a HIP device ordinal); holds the device table and the chunk sums of the last bind */
int tamf_optim_create(int32_t device, void** out_handle);
void tamf_optim_destroy(void* handle);

/* (Re)build the device table of n tensors: the pointer quadruples p[i], g[i], exp_avg[i], exp_avg_sq[i] of numel[i] floats each,
 * and the chunk table (tensor, chunk in tensor) at TAMF_OPTIM_CHUNK elements per chunk.  Call again whenever a pointer changes.
 * n >= 0; numel[i] >= 0 (a tensor of 0 elements has no chunk and is never touched); a null p or g of a tensor with elements is
 * TAMF_ERR_INVALID.  exp_avg[i] and exp_avg_sq[i] may both be null (a tensor that has no optimiser state yet): such a table serves
 * tamf_optim_grad_norms only, and tamf_optim_step on it is TAMF_ERR_STATE.  Host arrays, read before the call returns.
 * Synchronises the device. */
int tamf_optim_bind(void* handle, int32_t n, const void* const* p, const void* const* g, const void* const* exp_avg,
                    const void* const* exp_avg_sq, const int64_t* numel);

/* out_dev[i] = sqrt(sum g[i]^2) for the n bound tensors (0 for an empty one), n floats of device memory; two launches */
int tamf_optim_grad_norms(void* handle, float* out_dev, void* stream);

/* One clip + AdamW step of every bound tensor; max_norm < 0: no clipping.  step_index >= 1 is the step being taken (torch's
 * state["step"] after its increment).  lr, beta1, beta2, eps, weight_decay as torch.optim.AdamW names them; 0 <= beta < 1. */
int tamf_optim_step(void* handle, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                    int64_t step_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_OPTIM_H */
