// b^t in fp64 by square and multiply - the power behind Adam's bias corrections 1 - beta^t (head_train.hip, adam.hip; restated in
// numpy by tests/_adam_ref.py).  A function of (b, t) alone: a run that starts at step t gets the bits of one that ran through it.
#pragma once
#include <hip/hip_runtime.h>

namespace wdg {

__host__ __device__ __forceinline__ double ipow_f64(double b, int t) {
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

}  // namespace wdg
