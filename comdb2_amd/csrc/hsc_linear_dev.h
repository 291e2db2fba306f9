// hsc_linear_dev.h -- what the two tiers of the linearizability search share on
// the device (hsc_linear.hip, hsc_linear_wide.hip): the hash of
// a configuration word and the cas-register model's step.
#pragma once
#include "hsc_internal.h"

namespace hsc {

__device__ __forceinline__ uint32_t lin_hash(uint64_t key)
{
    uint32_t h = (uint32_t)key * 0x9E3779B1u ^ (uint32_t)(key >> 32) * 0x85EBCA6Bu;
    return h ^ h >> 15;
}

// The op (f, a, b) on state st: legal?  *ns: the state after it.
__device__ __forceinline__ bool lin_apply(uint32_t f, uint32_t a, uint32_t b, uint32_t st, uint32_t *ns)
{
    if (f == HSC_LIN_WRITE) {
        *ns = a;
        return true;
    }
    if (f == HSC_LIN_CAS) {
        *ns = b;
        return st == a;
    }
    *ns = st;  // a read: nil (id 0) matches any state
    return a == 0 || a == st;
}

}  // namespace hsc
