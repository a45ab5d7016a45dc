// rt_error.h — the library's error channel: the error of the calling thread's last failed call (rt_last_error).  Plain C++.
#pragma once
#include <string>

namespace rt {

inline thread_local std::string g_err;
inline int set_err(int st, const std::string& msg) {
    g_err = msg;
    return st;
}

}  // namespace rt
