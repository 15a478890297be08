// emdr2_amd/csrc/device_attr.h -- host-side facts and opt-ins that belong to a DEVICE, not to the process: the compute-unit count, and the
// dynamic-LDS opt-in of a kernel that asks for more than the 64 KB it gets without asking.
#ifndef EMDR2_DEVICE_ATTR_H
#define EMDR2_DEVICE_ATTR_H
#include <hip/hip_runtime.h>
#include <mutex>

#define EMDR2_MAX_DEVICES 64

// compute units of the current device (256 when it cannot be asked)
inline int device_cu_count()
{
    static std::mutex lock;
    static int cus[EMDR2_MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EMDR2_MAX_DEVICES) return 256;
    std::lock_guard<std::mutex> guard(lock);
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return 256;
        cus[dev] = n;
    }
    return cus[dev];
}

enum LdsOptIn { LDS_OPT_IN_OK = 0, LDS_OPT_IN_BELOW_REQUEST, LDS_OPT_IN_REFUSED };

// Lets Kernel use `bytes` of dynamic LDS on the current device.  The attribute belongs to (function, device): one flag per device ordinal, set
// under a lock (callers may be threads of several devices).  A device whose opt-in limit is below the request (not gfx950) is reported apart
// from a runtime that refuses: to some callers the first is an unsupported shape, not an error.
// Every caller asks for ONE size per kernel (a constexpr of its launcher): the flag remembers that the opt-in was made, not for how much.
template <auto Kernel>
int lds_opt_in(int bytes)
{
    static std::mutex lock;
    static bool done[EMDR2_MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EMDR2_MAX_DEVICES) return LDS_OPT_IN_REFUSED;
    std::lock_guard<std::mutex> guard(lock);
    if (done[dev]) return LDS_OPT_IN_OK;
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) limit = 0;
    if (limit > 0 && limit < bytes) return LDS_OPT_IN_BELOW_REQUEST;
    if (hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return LDS_OPT_IN_REFUSED;
    }
    done[dev] = true;
    return LDS_OPT_IN_OK;
}
#endif
