// The device check in front of every entry point that takes a device id (api.hip, test_hooks.hip).
#pragma once
#include <cstring>
#include <string>

#include "../../include/kokorox_hip.h"
#include "kx_common.h"

static inline void check_device(int device_id) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) throw kx::Error(KX_ERR_DEVICE, "no HIP device is visible (the HIP path has no CPU fallback)");
    if (device_id < 0 || device_id >= n) throw kx::Error(KX_ERR_INVALID, "device id out of range");
    hipDeviceProp_t p;
    KX_HIP(hipGetDeviceProperties(&p, device_id));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        throw kx::Error(KX_ERR_DEVICE, std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only");
}
