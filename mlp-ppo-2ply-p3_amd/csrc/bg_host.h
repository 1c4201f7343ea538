// bg_host.h — the host side of every C entry point: how a HIP error becomes a status.
// Host code only (no device code; needs nothing of hipcc beyond the runtime API header).
#pragma once
#include <hip/hip_runtime_api.h>

#include "../../include/bgx.h"

// Defined in bg_engine.hip.  bgx_internal_fail stores e's message for bgx_last_error()
// (per thread) and returns `code`; bgx_set_error stores a message of the caller's own.
int bgx_internal_fail(hipError_t e, int code = BGX_EDEVICE);
void bgx_set_error(const char* msg);

// The status of the launches issued so far: BGX_OK, or the failure with its message set.
inline int bgx_launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BGX_OK : bgx_internal_fail(e);
}

// Return from the entry point when a HIP call (BGX_CK) or an earlier launch (BGX_CK_LAUNCH) failed.
#define BGX_CK(x) do { const hipError_t _e = (x); if (_e != hipSuccess) return bgx_internal_fail(_e); } while (0)
#define BGX_CK_LAUNCH() BGX_CK(hipGetLastError())
