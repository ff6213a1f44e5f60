// Error plumbing shared by all translation units of libdia_hip.so.
#pragma once
#include <hip/hip_runtime.h>

int dia_fail(int code, const char* msg);
int dia_fail_hip(hipError_t e, const char* where);
// after a launch: a dynamic-LDS raise that failed (dia_launch skipped the launch), else hipGetLastError(); 0 when clean
int dia_check_launch(const char* kernel);
