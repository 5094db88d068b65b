// akr_path_forms.h — the names the host's render plan (path_plan.h) shares with the persistent path
// kernels: plain C++, no HIP header.  akr_device.h includes it, so device code sees them too.
#pragma once
#include <stdint.h>

namespace akr {

// persistent path kernel forms
enum : int { PATH_PLAIN = 0, PATH_DEFER = 1, PATH_SPEC = 2 };

// How fetch_pixels (kernels.hip) maps the i-th fetch of a shard to a slot of it (PathArgs::order_mode)
enum : uint32_t { FETCH_LINEAR = 0, FETCH_SCRAMBLE = 1, FETCH_PAIR = 2, FETCH_STRIDE = 3 };

}  // namespace akr
