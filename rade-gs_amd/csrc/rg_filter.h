// rg_filter.h -- the flag / scan / counts half of mesh compaction, which radegs_tetmesh.hip (vertex flags decide the faces) and
// radegs_meshclean.hip (face flags decide the vertices) share.  Defined in radegs_tetmesh.hip.  Layout: flags[0, NV) the vertices, flags[NV, NV + NF)
// the faces; incl is the inclusive scan of both, so a kept vertex v becomes incl[v] - 1 and a kept face f becomes incl[NV + f] - incl[NV - 1] - 1.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace rg {

struct FilterView {
  uint32_t *flags, *incl;
  void* temp;
  size_t temp_bytes, bytes;
};
FilterView filter_carve(long long NV, long long NF, void* base);   // a null base: only .bytes
bool filter_sizes_ok(long long NV, long long NF);
// with w.flags written: the scan, then counts2 = {kept vertices, kept faces} on the device
int filter_scan_counts(long long NV, long long NF, const FilterView& w, long long* counts2, hipStream_t s);

}  // namespace rg
