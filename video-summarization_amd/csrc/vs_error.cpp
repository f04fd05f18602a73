// vs_error.cpp - the calling thread's last error text (vs_error.h): set by every C ABI file, read by vs_last_error().
#include "vs_error.h"

#include <string>

namespace {
thread_local std::string g_err;
}

int vs_fail_msg(int code, const char *msg) { g_err = msg; return code; }

extern "C" const char *vs_last_error(void) { return g_err.c_str(); }
