// The library's one error report: never abort, return a code and keep a message for the calling thread.  Every
// ace_*_last_error of include/ace_sfno.h reads the same string (errors.cpp).  Host code only.
#pragma once
#include <string>

namespace ace {

int fail(int code, const std::string& msg);   // stores msg for this thread, returns code
const char* last_error();                     // this thread's message; valid until its next fail()

}  // namespace ace

// a HIP call that failed: its text and the runtime's reason, ACE_ERR_RUNTIME
#define ACE_HIP_TRY(expr)                                                                                              \
    do {                                                                                                               \
        hipError_t e__ = (expr);                                                                                       \
        if (e__ != hipSuccess) return ace::fail(ACE_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
// a library call that failed has left its message: pass its code on
#define ACE_TRY(expr)                    \
    do {                                 \
        int rc__ = (expr);               \
        if (rc__ != ACE_OK) return rc__; \
    } while (0)
