// What the optimizer's kernels (optim.hip) and the training meters (meters.hip) must agree on: the poly learning-rate schedule and how the control
// block of include/lavt_hip.h ("Control block `ctl`", LAVT_CTL_*) is read.  One definition each, so that a new slot or a changed rule has one place.
#pragma once
#include "common.h"

// lr = base lr * this, k = the device step counter (applied updates so far).  The update and the meter's logged lr evaluate the same expression.
__device__ __forceinline__ float poly_lr_factor(float k, float total_steps, float power) {
    return total_steps > 0.f ? powf(fmaxf(1.f - k / total_steps, 0.f), power) : 1.f;
}

// "This launch must leave everything alone", in the two forms the kernels use.  Both are wave-uniform reads, taken before the first store.
//   cycle open:      hold (host-written) or accumulating (this micro-step does not end its cycle) -- what the LAST cycle left in ctl stays valid
//   update blocked:  skip, or the cycle is open -- the update itself must not happen
// Two sites read FEWER slots on purpose and therefore use neither: lavt_grad_norm's passes look at accumulating only (under hold the norm is still
// computed and written), lavt_grad_accumulate's fold looks at hold only (it is the writer of accumulating).  The guarded tick and the meter tell
// the slots apart.  Each of them reads ctl[LAVT_CTL_...] directly, with its reason beside it.
__device__ __forceinline__ bool ctl_cycle_open(const float* ctl) { return ctl[LAVT_CTL_HOLD] != 0.f || ctl[LAVT_CTL_ACCUMULATING] != 0.f; }
__device__ __forceinline__ bool ctl_update_blocked(const float* ctl) { return ctl[LAVT_CTL_SKIP] != 0.f || ctl_cycle_open(ctl); }
