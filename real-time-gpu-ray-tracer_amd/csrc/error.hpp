// error.hpp — the thread-local message behind rt_last_error() (rt_api.cpp), for every host file; needs no HIP
#pragma once

#include <string>

void rtamd_set_error(const std::string &msg);
