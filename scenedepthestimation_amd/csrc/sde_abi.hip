// sde_abi.hip -- the library-wide ABI functions of include/sde.h (host only: no kernels).
#include "sde.h"

#define SDE_EXPORT extern "C" __attribute__((visibility("default")))   // as sde_common.h (HIP, not included here)

SDE_EXPORT int sde_abi_version(void) { return SDE_ABI_VERSION; }

SDE_EXPORT const char *sde_status_string(int s)
{
    switch (s) {
    case SDE_OK: return "ok";
    case SDE_ERR_ARG: return "invalid argument";
    case SDE_ERR_LAUNCH: return "kernel launch failed";
    case SDE_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown status";
    }
}
