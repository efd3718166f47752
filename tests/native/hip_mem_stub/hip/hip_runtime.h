/* A stand-in for <hip/hip_runtime.h> that keeps "device" memory on the HOST (tests/native/workspace_registry_check.cpp): what
 * dusp_amd/csrc/abi_internal.hpp needs to compile and what its DevBuf and dusp_program call — hipMalloc / hipFree / hipMemset / hipMemcpy
 * onto malloc / free / memset / memcpy, hipSetDevice and hipGetErrorString, and (the program's destructor) hipHostFree and hipEventDestroy.
 * Guard bytes behind a workspace are then host bytes a test can flip, under AddressSanitizer.  (hip_host_stub beside this one is for kernels.) */
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef void *hipStream_t;
typedef void *hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
static inline hipError_t hipMalloc(void **p, size_t n) { return (*p = std::malloc(n ? n : 1)) ? hipSuccess : hipErrorOutOfMemory; }
static inline hipError_t hipFree(void *p) { std::free(p); return hipSuccess; }
static inline hipError_t hipMemset(void *p, int value, size_t n) { std::memset(p, value, n); return hipSuccess; }
static inline hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) { std::memcpy(dst, src, n); return hipSuccess; }
static inline hipError_t hipSetDevice(int) { return hipSuccess; }
static inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
static inline hipError_t hipHostFree(void *p) { std::free(p); return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
