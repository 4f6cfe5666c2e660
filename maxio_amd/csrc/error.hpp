// error.hpp — the calling thread's last error (runtime.cpp) and the early
// return on it.  No HIP: the host-only units include this, not runtime.hpp.
#pragma once

#include <string>

#include "../../include/maxio_ec.h"

namespace mxec {

int set_error(int code, const std::string& msg);
const char* last_error();

}  // namespace mxec

#define MXEC_TRY(expr)              \
    do {                            \
        int _rc = (expr);           \
        if (_rc != MXEC_OK) return _rc; \
    } while (0)
