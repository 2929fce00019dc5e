// The error message of a library: a per-thread buffer that lbdrn::set_error writes and lbdrn::last_error() returns (both
// declared in common.hpp).  Included by exactly one translation unit of each shared library -- generic.hip for
// liblbdrn_hip.so, the one .hip file of every other -- so each library has a buffer of its own (hidden visibility).
#include <stdarg.h>
#include <stdio.h>

namespace lbdrn {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

const char* last_error() { return g_error; }

}  // namespace lbdrn
