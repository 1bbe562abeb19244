// mpc_host.h -- the host plumbing every part of the MPC data path uses (mpc_linearise.hip,
// mpc_assembly.hip, mpc_device.hip): the device-call guard, the upload of a host vector, and the one way a kernel
// is launched.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/mpcqp.h"
#include "kernels.h"

#define MHIPCHK(expr)                                                                        \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return set_error(MPCQP_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

namespace mpcqp {

template <class T>
int upload(const std::vector<T>& v, T** d) {
    MHIPCHK(hipMalloc((void**)d, sizeof(T) * std::max<size_t>(v.size(), 1)));
    if (!v.empty()) MHIPCHK(hipMemcpy(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return 0;
}

inline unsigned grid_of(long count, int block) { return (unsigned)((count + block - 1) / block); }

// hipSetDevice, one launch of `count` threads in blocks of `block`, hipGetLastError
template <class... P, class... A>
int launch(int device, void* stream, long count, int block, void (*kernel)(P...), A... args) {
    MHIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(kernel, dim3(grid_of(count, block)), dim3(block), 0, (hipStream_t)stream, (P)args...);
    MHIPCHK(hipGetLastError());
    return 0;
}

}  // namespace mpcqp
