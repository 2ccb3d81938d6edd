// What a translation unit beside evac_api.hip needs of a handle (evac_deepsets_api.hip: entries that take one).  The handle's
// struct stays evac_api.hip's own; these four functions are defined there and are not exported from the library.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/evac.h"
#include "evac_common.h"

namespace evac_host {

struct HandleView {
    evac::Params p;
    int device;
    bool default_cfg;       // the configuration the specialised (DEF) kernels assume
};

#define EVAC_HOST_LOCAL __attribute__((visibility("hidden")))
// What every entry with a handle checks first (a NULL handle, unbound state, a lost team): EVAC_OK and `out` filled, or the code
EVAC_HOST_LOCAL int handle_begin(evac_handle_t h, const char* what, HandleView* out);
// Handles with parts = 2 or chain = 1 / 2 are joined: `stream` waits for their own streams
EVAC_HOST_LOCAL int handle_settle(evac_handle_t h, hipStream_t stream);
// `msg` becomes evac_last_error(h); returns `code`
EVAC_HOST_LOCAL int handle_fail(evac_handle_t h, int code, const std::string& msg);
EVAC_HOST_LOCAL int handle_check_launch(evac_handle_t h, const char* what);
#undef EVAC_HOST_LOCAL

}  // namespace evac_host
