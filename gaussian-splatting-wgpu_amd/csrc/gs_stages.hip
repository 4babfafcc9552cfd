// gs_stages.hip -- the two stand-alone stages of the C ABI (include/gsplat/gs_abi.h): the radix sort and the exclusive scan on
// host arrays, without a context (the host halves of GPUSorter, reference src/radix_sort/sort.ts:249-350, and ExclusiveScanner,
// src/exclusive_scan.ts:208-325).  Their device arrays are local owners: every exit frees them.
#include <cstddef>

#include "gs_runtime.h"

GS_EXPORT int32_t gs_sort_pairs_u32(int32_t device, uint32_t* keys, uint32_t* values, uint64_t n, uint32_t key_bits) {
    if (!keys && n) return fail(GS_ERR_INVALID_ARGUMENT, "gs_sort_pairs_u32: null keys");
    if (n >= (1ull << 30)) return fail(GS_ERR_CAPACITY, "gs_sort_pairs_u32: n >= 2^30");
    if (key_bits == 0 || key_bits > 32) key_bits = 32;
    if (n == 0) return GS_OK;
    HIP_TRY(hipSetDevice(device));
    const uint32_t passes = (key_bits + 7) / 8;
    const size_t kb = (size_t)n * 4, ctl_bytes = private_sort_bytes(n, passes);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    DevBuf<uint32_t> kA, vA, kB, vB;
    DevBuf<> ctl_mem;
    HIP_TRY(hipMalloc(kA.out(), kb)); HIP_TRY(hipMalloc(vA.out(), kb)); HIP_TRY(hipMalloc(kB.out(), kb)); HIP_TRY(hipMalloc(vB.out(), kb));
    HIP_TRY(hipMalloc(ctl_mem.out(), ctl_bytes));
    HIP_TRY(hipMemset(ctl_mem, 0, ctl_bytes));
    HIP_TRY(hipMemcpy(kA, keys, kb, hipMemcpyHostToDevice));
    if (values) HIP_TRY(hipMemcpy(vA, values, kb, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(vA, 0, kb));
    GsControl* ctl = (GsControl*)ctl_mem.get(); // view into ctl_mem; the sort's status words follow it
    const uint32_t n32 = (uint32_t)n;
    HIP_TRY(hipMemcpy(&ctl->num_intersections, &n32, 4, hipMemcpyHostToDevice));
    const GsSortPair sorted = gs_launch_sort(private_sort_plan(kA, vA, kB, vB, passes), ctl, (uint32_t*)((char*)ctl_mem.get() + kCtlBytes), n32,
                                             (uint32_t)prop.multiProcessorCount * 4, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    uint32_t fault = 0;
    HIP_TRY(hipMemcpy(&fault, &ctl->fault, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(keys, sorted.keys, kb, hipMemcpyDeviceToHost));
    if (values) HIP_TRY(hipMemcpy(values, sorted.vals, kb, hipMemcpyDeviceToHost));
    if (fault) return fail(GS_ERR_DEVICE_FAULT, "gs_sort_pairs_u32: look-back spin bound exceeded");
    return GS_OK;
}

GS_EXPORT int32_t gs_exclusive_scan_u32(int32_t device, uint32_t* data, uint64_t n, uint64_t* total) {
    if ((!data && n) || !total) return fail(GS_ERR_INVALID_ARGUMENT, "gs_exclusive_scan_u32: null argument");
    if (n >= (1ull << 31)) return fail(GS_ERR_INVALID_ARGUMENT, "gs_exclusive_scan_u32: n too large");
    *total = 0;
    if (n == 0) return GS_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t kb = (size_t)n * 4;
    const size_t ctl_sz = kCtlBytes, st_sz = ((size_t)gs_scan_blocks((uint32_t)n) + 1) * 8;
    DevBuf<uint32_t> in, out;
    DevBuf<> ctl_mem;
    HIP_TRY(hipMalloc(in.out(), kb)); HIP_TRY(hipMalloc(out.out(), kb)); HIP_TRY(hipMalloc(ctl_mem.out(), ctl_sz + st_sz));
    HIP_TRY(hipMemset(ctl_mem, 0, ctl_sz + st_sz));
    HIP_TRY(hipMemcpy(in, data, kb, hipMemcpyHostToDevice));
    GsControl* ctl = (GsControl*)ctl_mem.get(); // view into ctl_mem; the scan's status words follow it
    gs_launch_scan(in, (uint32_t)n, out, (unsigned long long*)((char*)ctl_mem.get() + ctl_sz), &ctl->scan_ticket[0], ctl, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    GsControl h;
    HIP_TRY(hipMemcpy(&h, ctl, offsetof(GsControl, hist), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data, out, kb, hipMemcpyDeviceToHost));
    if (h.fault) return fail(GS_ERR_DEVICE_FAULT, "gs_exclusive_scan_u32: look-back spin bound exceeded");
    *total = h.num_intersections;
    return GS_OK;
}
