// msda_host.h -- the host side every translation unit of the library shares (internal; not part of the C ABI).
//
// ONE RULE: an exported function that returns non-zero has set the text behind msda_last_error() in that same call, through one of
// the three *fail functions below -- so the text always belongs to the call that failed, never to an earlier one.  The functions are
// defined once, in msda_api.hip (which owns the thread-local text), with hidden visibility.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/richsem_msda.h"

namespace msda {

// sets the text (printf format) and returns `code`
__attribute__((visibility("hidden"), format(printf, 2, 3))) int fail(int code, const char *fmt, ...);

// a failed argument check: "<entry point>: <class of error>" for an MSDA_ERR_* code; returns `code`
__attribute__((visibility("hidden"))) int arg_fail(int code, const char *entry);

// a failed runtime call: "<what><tag>: <hipGetErrorString> (hipError N)"; returns (int)e.  `what` is the entry point's name or says what
// was being done.
__attribute__((visibility("hidden"))) int hip_fail(hipError_t e, const char *what, const char *tag = "");

// after the launches of a call: MSDA_OK, or hip_fail of what hipGetLastError() holds
__attribute__((visibility("hidden"))) int launched(const char *what, const char *tag = "");

// Raise a kernel's dynamic-LDS limit.  Done once per (device, kernel, size class): repeating the runtime call on every
// launch costs time and is not something to issue while the caller captures its stream into a graph.
__attribute__((visibility("hidden"))) hipError_t set_lds_limit(const void *fn, size_t bytes);

// are all of `ptrs` multiples of `bytes` (a power of two)?  A null pointer counts as aligned: optional arguments go in as they are.
inline bool aligned(size_t bytes, std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & (bytes - 1)) == 0;
}

}  // namespace msda
