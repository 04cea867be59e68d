// rt_internal.h -- shared between the library's translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

// Sets the thread-local message rt_last_error returns; returns `code`.
int rt_internal_fail(int code, const std::string& msg);
// RT_OK when `device` is a visible gfx950 device (hipSetDevice done), else RT_E_NODEVICE/RT_E_HIP.
int rt_internal_use_device(int device, int *num_cus);

// The grid build's LSD radix sort (rt_grid_build.hip: 64-bit keys, 8 bits a pass, stable) for the other
// translation units (rt_trace_rays_device's RT_RAYS_SORT), over device scratch that is kept between calls
// and reallocated only when n exceeds every earlier n (a reallocation frees, which waits for the device).
struct rt_sort_scratch;
// *keys = a buffer of >= n keys for the caller to fill on the stream it then sorts on
int rt_internal_sort_reserve(rt_sort_scratch **sc, uint32_t n, unsigned long long **keys);
// Sorts the n keys by their low `bits` bits on st (asynchronous); *sorted = the result, inside the scratch.
int rt_internal_sort_run(rt_sort_scratch *sc, hipStream_t st, uint32_t n, uint32_t bits, unsigned long long **sorted);
void rt_internal_sort_free(rt_sort_scratch *sc);
