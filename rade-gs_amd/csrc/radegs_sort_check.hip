// radegs_sort_check.hip -- test-only C entry points over the hand-written device-wide primitives of csrc/radegs_sort.hip (rg_prims.h), with the
// instantiation override exposed.  Linked with radegs_sort.o into libradegs_sort_check.so (build.py), next to libradegs_prims_check.so; never part of
// libradegs_hip.so.  Loaded with ctypes by tests/test_gpu_sort_scan.py.  Every call returns the hipError_t as an int; nothing synchronises.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rg_prims.h"

extern "C" {

size_t sortcheck_sort_temp_bytes(size_t n) { return rg::sort_temp_bytes(n); }
size_t sortcheck_scan_temp_bytes(size_t n) { return rg::scan_temp_bytes(n); }

int sortcheck_sort_u32(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                       size_t n, int end_bit, void* stream, const uint32_t* n_dev, int items) {
  return (int)rg::radix_sort_pairs_u32(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, (hipStream_t)stream, n_dev, items);
}

int sortcheck_sort_u16(void* temp, size_t temp_bytes, const uint16_t* keys_in, uint16_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                       size_t n, int end_bit, void* stream, const uint32_t* n_dev, int items) {
  return (int)rg::radix_sort_pairs_u16(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, (hipStream_t)stream, n_dev, items);
}

int sortcheck_sort_u32_27(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                          size_t n, uint32_t key_base, void* stream, int items) {
  return (int)rg::radix_sort_pairs_u32_27(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, key_base, (hipStream_t)stream, items);
}

// Two entry points, because a C symbol cannot take an optional argument: a caller written for the 14-argument form would leave `joined` to
// whatever the stack holds, and the sort would write there.  The first keeps that form (no joined key), the second passes the pointer through
// (null allowed).
int sortcheck_sort_2xu32(void* temp, size_t temp_bytes, const uint32_t* minor, const uint32_t* major, uint32_t* major_sorted, uint32_t* perm,
                         uint32_t* s0, uint32_t* s1, uint32_t* s2, size_t n, int minor_end_bit, int major_end_bit, void* stream,
                         const uint32_t* n_dev) {
  return (int)rg::radix_sort_order_2xu32(temp, temp_bytes, minor, major, major_sorted, perm, s0, s1, s2, n, minor_end_bit, major_end_bit,
                                         (hipStream_t)stream, n_dev);
}
int sortcheck_sort_2xu32_joined(void* temp, size_t temp_bytes, const uint32_t* minor, const uint32_t* major, uint32_t* major_sorted, uint32_t* perm,
                                uint32_t* s0, uint32_t* s1, uint32_t* s2, size_t n, int minor_end_bit, int major_end_bit, void* stream,
                                const uint32_t* n_dev, unsigned long long* joined) {
  return (int)rg::radix_sort_order_2xu32(temp, temp_bytes, minor, major, major_sorted, perm, s0, s1, s2, n, minor_end_bit, major_end_bit,
                                         (hipStream_t)stream, n_dev, joined);
}

int sortcheck_scan(void* temp, size_t temp_bytes, const uint32_t* vals, const uint32_t* idx, uint32_t* out, size_t n, void* stream,
                   uint32_t* packed_out, unsigned long long* sq_sum, int items) {
  return (int)rg::inclusive_scan_gather_u32(temp, temp_bytes, vals, idx, out, n, (hipStream_t)stream, packed_out, sq_sum, items);
}

}  // extern "C"
