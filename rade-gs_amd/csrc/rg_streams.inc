// rg_streams.inc -- blend kernels over SUB-TILE ENTRY STREAMS (included by radegs_kernels.hip; needs its helpers in scope).
//
//   renderCUDA fwd   DGR/cuda_rasterizer/forward.cu:428-693    -> block_lists_kernel + blend_fwd_streams_kernel
//   renderCUDA bwd   DGR/cuda_rasterizer/backward.cu:631-1016  -> blend_bwd_streams_kernel
//
// Why a second formulation.  A wave iteration of the blend loops costs the same whether 1 or 64 lanes blend, and on scenes of
// small splats (C2: a splat's {alpha >= 1/255} footprint is ~160 px, ~34 px inside a 16x16 tile) most lanes of a tile-wide
// walk idle.  Here every 16x16 tile is cut into 8 blocks of 8x4 pixels; the instance emission (emit_instances_kernel<true>) tests
// every (tile, Gaussian) instance against the tile's 8 blocks by the geometry of the splat's {alpha >= 1/255} ellipse itself, not
// its bounding box (ellipse_tile_mask, rg_blend.h), the 8-bit answer rides through the tile sort in the top byte of the instance
// value, and block_lists_kernel turns every sorted tile list into 8 depth-ordered sub-lists.  A wave owns a 16x8 strip = 4 blocks; each 16-lane DPP
// row walks the list of ITS block (2 pixels per lane, rows 2 apart) one entry per iteration:
//   * no per-iteration bookkeeping -- the lists are already culled, every row consumes exactly one entry per step, the wave
//     runs max-over-rows(list length) iterations in total (C2-like scene: 141 per strip instead of 170 with in-kernel
//     bounding-box culls whose per-batch maxima add up, 256 with one stream per wave);
//   * the loop body is straight-line predicated code (with four different entries in flight some lane is always a candidate,
//     so wave-uniform skips never trigger);
//   * the forward records, per lane and round of 16 entries, one word of "this pixel blended entry j" bits; the backward replays
//     the forward's decisions from those bits: no exponent thresholds, no exp_spec, no last-contributor compares (the
//     quadratic form itself is still evaluated in the forward's order of operations -- needle-thin splats need it);
//   * per-Gaussian sums are reduced inside the row (4 DPP stages) and leave as ONE 16-lane atomic line update per
//     (block, entry).
// Storage: ImageState::blk_* (rg_layout.h), round chunks of 16 entries.
//
// Selected per launch (rg_launch.inc: use_streams) for small-splat scenes; the tile-wide kernels above stay for large splats,
// where every entry reaches every block and sub-lists would only multiply the list traffic.

namespace rg {

constexpr int kGrpSlots = 17;   // LDS slots per row: the rows read slot j in lockstep -> +1 keeps them on different bank quads
constexpr uint32_t kNoPos = 0xFFFFFFFEu;

struct BlockListArgs {
  const uint2* ranges; uint32_t* point_list;
  const uint32_t* keys_sorted;   // MASK_IN_KEY: the sorted 32-bit tile keys, block mask in the top byte
  int gx, ntiles;
  uint32_t* blk_count; uint32_t* blk_base; uint32_t* blk_chunks;
  uint32_t* wg_need;             // [grid] chunks the tiles of each workgroup need (block_counts_kernel -> block_lists_kernel)
  uint32_t* stream_meta;         // ImageState::stream_tag: [1] chunks the lists need in all, [3] set when the capacity did not suffice
  uint32_t chunk_capacity;       // chunks of kChunkWords words blk_chunks holds
  // block_lists_kernel only: its first `bal_groups` workgroups sort the blocks of a 64-tile neighbourhood by list length (balance_blocks),
  // the `list_grid` that follow build the lists; the last of those reports to the host's mapped words (may be null) and publishes `seq`
  int list_grid, bal_groups;
  uint32_t* blk_order; uint32_t* pin_chunks; uint32_t* pin_seq; uint32_t seq;
};

// The sub-lists are stored back to back at their real size (round 5; rounds 2-4 reserved the tile's WHOLE list for every block -- 8 x
// ceil(n/16) chunks per tile, ~96 B per instance of capacity, C2: 0.48 GB for 0.11 GB of lists -- which needed no count but made the
// image state 3x the reference's and capped the scene size the streams could take: VERDICT r4, item 5).  Two kernels over the same
// grid, workgroup w owning the tiles w, w + G, w + 2G, ... (in XCD band order):
//   block_counts_kernel   per tile: how many entries each of the 8 blocks gets (the top byte of every list word -- or of its sorted
//                         key: MASK_IN_KEY, scenes of 2^24 Gaussians and more -- says which blocks the entry can reach,
//                         emit_instances_kernel<true>) -> blk_count, and the chunks the workgroup's tiles need in all -> wg_need[w].
//   block_lists_kernel    the workgroup adds up wg_need[0 .. w) itself (a few KB from L2: no scan kernel, no atomic -- one allocator
//                         word served 8 160 returning atomics at ~8 ns each: +0.07 ms) -- its tiles' lists start there, tile after
//                         tile, block after block -- and appends.
// Tiles whose chunks would not fit the capacity get empty lists and raise stream_meta[3] (the host redoes the forward, rg_launch.inc).
constexpr int kListThreads = 256;
template <bool MASK_IN_KEY>
__global__ void __launch_bounds__(kListThreads) block_counts_kernel(const BlockListArgs a) {
  __shared__ uint32_t tile_cnt[2][4][kBlocksPerTile];   // every wave's per-block totals over the tile list (double-buffered: one barrier per tile)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = (int)gridDim.x;
  auto range_of = [&](int i) { return i < a.ntiles ? a.ranges[xcd_band_remap(i, a.ntiles)] : make_uint2(0u, 0u); };
  auto mask_at = [&](uint32_t pos) -> uint32_t { return (MASK_IN_KEY ? a.keys_sorted[pos] : a.point_list[pos]) >> kMaskShift; };
  uint2 r_cur = range_of((int)blockIdx.x), r_nxt = range_of((int)blockIdx.x + G);
  uint32_t keep_first = (uint32_t)tid < r_cur.y - r_cur.x ? mask_at(r_cur.x + tid) : 0u;
  uint32_t need_wg = 0u;
  int buf = 0;
  for (int it = blockIdx.x; it < a.ntiles; it += G, buf ^= 1) {
    const int tile = xcd_band_remap(it, a.ntiles);
    const uint2 range = r_cur;
    const uint32_t n = range.y - range.x;
    const uint2 r_nn = range_of(it + 2 * G);
    const uint32_t keep_first_nxt = (uint32_t)tid < r_nxt.y - r_nxt.x ? mask_at(r_nxt.x + tid) : 0u;
    uint32_t cnt[kBlocksPerTile];   // this wave's entries per block (wave-uniform)
#pragma unroll
    for (int b = 0; b < kBlocksPerTile; b++) cnt[b] = 0u;
    uint32_t keep = keep_first;
    for (uint32_t base = 0; base < n; base += kListThreads) {
      const uint32_t k_next = base + kListThreads + tid;
      const uint32_t keep_n = k_next < n ? mask_at(range.x + k_next) : 0u;
#pragma unroll
      for (int b = 0; b < kBlocksPerTile; b++) cnt[b] += (uint32_t)__popcll(__ballot((keep >> b) & 1u));
      keep = keep_n;
    }
    if (lane == 0) {
#pragma unroll
      for (int b = 0; b < kBlocksPerTile; b++) tile_cnt[buf][wave][b] = cnt[b];
    }
    __syncthreads();
    if (tid < kBlocksPerTile) {
      const uint32_t c = tile_cnt[buf][0][tid] + tile_cnt[buf][1][tid] + tile_cnt[buf][2][tid] + tile_cnt[buf][3][tid];
      a.blk_count[(size_t)tile * kBlocksPerTile + tid] = c;
      uint32_t ch = (c + 15u) >> 4;   // chunks of this block; summed over the 8 lanes below
      ch += __shfl_xor(ch, 1); ch += __shfl_xor(ch, 2); ch += __shfl_xor(ch, 4);
      need_wg += ch;                   // (lanes 0..7 of wave 0 all hold the tile's total)
    }
    r_cur = r_nxt; r_nxt = r_nn; keep_first = keep_first_nxt;
  }
  if (tid == 0) a.wg_need[blockIdx.x] = need_wg;
}

// Which four blocks share a wave.  The wave runs max-over-its-rows(list length) iterations, so rows of equal length waste nothing:
// inside every neighbourhood of 64 tiles (512 blocks, consecutive in the XCD band order the blend kernels walk, so the splat
// records stay in that XCD's L2) the blocks are sorted by list length, longest first, and consecutive quadruples form the waves
// (C2: 133.8 iterations per wave instead of 140.6 for the four blocks of a 16x8 strip; the mean list has 133.7 entries).
// Needs the blocks' counts only (block_counts_kernel), not the lists: since round 6 it runs in the FIRST workgroups of block_lists_kernel,
// next to the list building, instead of as a kernel of its own behind it (7.7 us + a kernel boundary per stream forward).
constexpr int kBalanceBlocks = 512;
static_assert(kListThreads == 256, "balance_blocks: one compare-exchange per thread per step over 512 keys, and strides of 256");
__device__ __forceinline__ void balance_blocks(int group, int nblocks, const uint32_t* __restrict__ blk_count, uint32_t* __restrict__ blk_order,
                                               uint64_t* keys /* LDS [kBalanceBlocks] */) {
  const int tid = threadIdx.x;
  const int base = group * kBalanceBlocks;
  if (base >= nblocks) return;   // (the launcher rounds the number of groups up to a multiple of 8)
  for (int e = tid; e < kBalanceBlocks; e += 256) {
    const int id = base + e;
    keys[e] = id < nblocks ? (((uint64_t)blk_count[id] + 1ull) << 32) | (uint64_t)(uint32_t)id : 0ull;   // padding sorts last
  }
  __syncthreads();
  for (int k = 2; k <= kBalanceBlocks; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int t = tid;   // 256 compare-exchanges per step
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      const int p = i | j;
      const uint64_t a = keys[i], b = keys[p];
      const bool down = (i & k) == 0;   // descending overall
      if ((a < b) == down) { keys[i] = b; keys[p] = a; }
      __syncthreads();
    }
  }
  for (int e = tid; e < kBalanceBlocks; e += 256)
    if (base + e < nblocks) blk_order[base + e] = (uint32_t)keys[e];
}

template <bool MASK_IN_KEY>
__global__ void __launch_bounds__(kListThreads) block_lists_kernel(const BlockListArgs a) {
  __shared__ uint2 wave_cnt[2][4];   // per wave: its 8 per-block counts of the step, one byte each (a wave holds 64 entries)
  __shared__ uint32_t red[4];
  __shared__ uint64_t bal_keys[kBalanceBlocks];
  if ((int)blockIdx.x < a.bal_groups) {   // (workgroup-uniform)
    balance_blocks((int)blockIdx.x, a.ntiles * kBlocksPerTile, a.blk_count, a.blk_order, bal_keys);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int buf = 0;
  const int G = a.list_grid;
  const int lidx = (int)blockIdx.x - a.bal_groups;   // this workgroup among the list builders: what block_counts_kernel's blockIdx was
  // ---- where this workgroup's lists start: the chunks of the workgroups before it (and, for the last one, the total) ----
  uint32_t before = 0u;
  for (int w = tid; w < lidx; w += kListThreads) before += a.wg_need[w];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d);
  if (lane == 0) red[wave] = before;
  // Grid-stride over the tiles (stride: a multiple of 8, so a workgroup's tiles stay in the band of the XCD it runs on).
  // Everything that is uniform over the wave -- the per-block counts, the positions reached so far, the list base addresses --
  // is kept on the scalar unit; the kernel is VALU-bound and every per-lane instruction saved counts.
  // The next tile's range and first 256 list words are requested while the current tile is processed (a tile is only two steps
  // long on C2: without this every tile starts with two dependent memory latencies that nothing covers).
  auto range_of = [&](int i) { return i < a.ntiles ? a.ranges[xcd_band_remap(i, a.ntiles)] : make_uint2(0u, 0u); };
  auto fetch_v = [&](const uint2 r, uint32_t k) -> uint32_t { return k < r.y - r.x ? a.point_list[r.x + k] : 0u; };
  auto fetch_m = [&](const uint2 r, uint32_t k) -> uint32_t { return (MASK_IN_KEY && k < r.y - r.x) ? a.keys_sorted[r.x + k] >> kMaskShift : 0u; };
  uint2 r_cur = range_of(lidx), r_nxt = range_of(lidx + G);
  uint32_t v_first = fetch_v(r_cur, (uint32_t)tid), m_first = fetch_m(r_cur, (uint32_t)tid);
  __syncthreads();
  uint32_t cursor = (uint32_t)__builtin_amdgcn_readfirstlane((int)(red[0] + red[1] + red[2] + red[3]));   // next free chunk
  if (lidx == G - 1 && tid == 0) {   // the lists' total need, for the host (a forward sized from the previous view's)
    const uint32_t total = cursor + a.wg_need[lidx];
    const uint32_t over = total > a.chunk_capacity ? 1u : 0u;
    a.stream_meta[1] = total;
    if (over) a.stream_meta[3] = 1u;
    // ... and straight to the host's mapped words: what the lists take from the chunk allocator, whether that exceeds what they were given,
    // and then -- release order -- the sequence number the host polls for (rg_launch.inc: PIN_CHUNKS, PIN_CHUNK_OVERFLOW, PIN_SEQ).
    // Both are known HERE, before a single list word is written; nothing the host does with them needs the lists.
    if (a.pin_chunks) {
      __hip_atomic_store(a.pin_chunks, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(a.pin_chunks + 1, over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(a.pin_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  for (int it = lidx; it < a.ntiles; it += G) {
    const int tile = xcd_band_remap(it, a.ntiles);
    const uint2 range = r_cur;
    const uint32_t n = range.y - range.x;
    const uint2 r_nn = range_of(it + 2 * G);
    const uint32_t v_first_nxt = fetch_v(r_nxt, (uint32_t)tid), m_first_nxt = fetch_m(r_nxt, (uint32_t)tid);
    // the blocks' counts (block_counts_kernel) -> their first chunks; a tile that does not fit leaves empty lists
    uint32_t chunks_before[kBlocksPerTile], need = 0u;
    {
      const uint4* pc = reinterpret_cast<const uint4*>(a.blk_count + (size_t)tile * kBlocksPerTile);
      const uint4 c0 = pc[0], c1 = pc[1];
      const uint32_t c[kBlocksPerTile] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int b = 0; b < kBlocksPerTile; b++) {
        chunks_before[b] = need;
        need += ((uint32_t)__builtin_amdgcn_readfirstlane((int)c[b]) + 15u) >> 4;
      }
    }
    const uint32_t tbase = cursor;
    cursor += need;
    const bool fits = tbase <= a.chunk_capacity && need <= a.chunk_capacity - tbase;
    if (tid < kBlocksPerTile) {
      uint32_t cb = 0u;
#pragma unroll
      for (int b = 0; b < kBlocksPerTile; b++) cb = tid == b ? chunks_before[b] : cb;
      a.blk_base[(size_t)tile * kBlocksPerTile + tid] = fits ? tbase + cb : 0u;
      if (!fits) a.blk_count[(size_t)tile * kBlocksPerTile + tid] = 0u;
    }
    if (fits && n) {
      char* const chunk0 = reinterpret_cast<char*>(a.blk_chunks + (size_t)tbase * kChunkWords);
      uint32_t run[kBlocksPerTile];   // entries appended to every block's list so far (wave-uniform)
#pragma unroll
      for (int b = 0; b < kBlocksPerTile; b++) run[b] = 0u;
      uint32_t v_n = v_first, m_n = m_first;
      for (uint32_t base = 0; base < n; base += kListThreads, buf ^= 1) {
        const uint32_t k = base + tid;
        const uint32_t gid = MASK_IN_KEY ? v_n : (v_n & kGidMask);
        const uint32_t keep = MASK_IN_KEY ? m_n : (v_n >> kMaskShift);   // bit b: block b (emit_instances_kernel<true>); 0 beyond the list
        v_n = fetch_v(range, k + kListThreads);
        m_n = fetch_m(range, k + kListThreads);
        if (!MASK_IN_KEY && k < n) a.point_list[range.x + k] = gid;   // from here on the list holds plain Gaussian indices, as the reference's does
        uint64_t m[kBlocksPerTile];
        uint32_t p0 = 0u, p1 = 0u;
#pragma unroll
        for (int b = 0; b < kBlocksPerTile; b++) {
          m[b] = __ballot((keep >> b) & 1u);
          const uint32_t c = (uint32_t)__popcll(m[b]);   // <= 64: a byte each, four to a word
          if (b < 4) p0 |= c << (8 * b); else p1 |= c << (8 * (b - 4));
        }
        if (lane == 0) wave_cnt[buf][wave] = make_uint2(p0, p1);
        __syncthreads();
        uint32_t w[4][2];
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const uint2 t = wave_cnt[buf][v];
          w[v][0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x);
          w[v][1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.y);
        }
#pragma unroll
        for (int b = 0; b < kBlocksPerTile; b++) {
          const int h = b >> 2, sh = 8 * (b & 3);
          const uint32_t c0 = (w[0][h] >> sh) & 255u, c1 = (w[1][h] >> sh) & 255u, c2 = (w[2][h] >> sh) & 255u, c3 = (w[3][h] >> sh) & 255u;
          const uint32_t before_w = run[b] + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);   // scalar
          if ((keep >> b) & 1u) {
            const uint32_t i = before_w + __builtin_amdgcn_mbcnt_hi((uint32_t)(m[b] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[b], 0u));
            const size_t off = (size_t)(chunks_before[b] + (i >> 4)) * (kChunkWords * sizeof(uint32_t)) + (i & 15u) * 8u;
            *reinterpret_cast<uint2*>(chunk0 + off) = make_uint2(gid, k);
          }
          run[b] += (c0 + c1) + (c2 + c3);
        }
      }
    }
    r_cur = r_nxt; r_nxt = r_nn; v_first = v_first_nxt; m_first = m_first_nxt;
  }
}

// wave-uniform maximum of a value that is uniform inside every 16-lane row
__device__ __forceinline__ uint32_t row_uniform_max(uint32_t v) {
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return max(max(a, b), max(c, d));
}

// The round's record gather, four lanes per record.  A lane that fetches its own entry's 64-byte record with four 16-byte loads makes
// every load instruction touch 64 different cache lines (a quarter of each): 256 line look-ups per wave and round.  Here instruction k
// fetches the 16 records of ROW k: lane i takes quarter (i & 3) of entry (i >> 2), so four neighbouring lanes cover one line and an
// instruction touches 16 lines -- 64 look-ups per round, every line exactly once.  The ids travel between the rows with ds_bpermute
// (LDS crossbar, no memory); the quarters land in LDS at the slot the per-lane staging used: lds[(k * row_stride + entry) * 4 + quarter].
// id == kNoId: nothing to fetch (past the end of the row's list) -> an all-zero record.
constexpr uint32_t kNoId = 0xFFFFFFFFu;
template <class V4>
__device__ __forceinline__ void gather_rows_to_lds(const float4* __restrict__ splat_a, uint32_t my_id, int lane, V4* lds, int row_stride_v4) {
  const int e = lane >> 2, qd = lane & 3;
  uint32_t idk[4];
#pragma unroll
  for (int k = 0; k < 4; k++) idk[k] = (uint32_t)__builtin_amdgcn_ds_bpermute((16 * k + e) << 2, (int)my_id);
  // byte offsets in 32 bits next to the scalar base (the launcher keeps scenes of 2^26 Gaussians and more off these kernels)
  const char* base = reinterpret_cast<const char*>(splat_a);
  float4 v[4];
#pragma unroll
  for (int k = 0; k < 4; k++)
    v[k] = idk[k] != kNoId ? *reinterpret_cast<const float4*>(base + ((idk[k] << 6) | ((uint32_t)qd << 4))) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 4; k++) lds[k * row_stride_v4 + e * 4 + qd] = V4{v[k].x, v[k].y, v[k].z, v[k].w};
}

// ---- set-up shared by the two stream kernels ----
// A 16-lane row of wave `item` owns one 8x4 block -- any block of the neighbourhood (balance_blocks, in block_lists_kernel), the same
// wave composition in the forward and the backward.  Lane l of the row holds pixel column px, rows py0 and py0 + 2.
constexpr int kStreamRowStep = 2;   // rows between the two pixels of one lane
struct StreamRow { uint32_t bid; int tile, blk, px, py0; };
__device__ __forceinline__ StreamRow stream_row_geometry(const uint32_t* blk_order, int item, int grp, int l, int gx) {
  StreamRow g;
  g.bid = blk_order[4 * (size_t)item + grp];
  g.tile = (int)(g.bid >> 3); g.blk = (int)(g.bid & 7u);
  const int tile_x = g.tile % gx, tile_y = g.tile / gx;
  const int brow = g.blk >> 1, bcol = g.blk & 1;
  g.px = tile_x * 16 + bcol * 8 + (l & 7);
  g.py0 = tile_y * 16 + brow * 4 + (l >> 3);
  return g;
}
// Lane l's list word of round r -- {Gaussian id, position in the tile list} -- of a list of n entries; {0, kNoPos} past its end.
// The backward, which asks one round ahead, ends with r = -1: as 0xFFFFFFFF its first position, 0xFFFFFFF0, lies past any list
// (n < 2^31: the tile list's length is an int), so the one compare covers that end too.
__device__ __forceinline__ uint2 load_list_word(const uint32_t* chunks, uint32_t r, int l, uint32_t n) {
  return (r * 16u + (uint32_t)l < n) ? *reinterpret_cast<const uint2*>(chunks + (size_t)r * kChunkWords + 2 * l) : make_uint2(0u, kNoPos);
}
// Coord-map mode: the 48-byte camera-plane record of the lane's entry (all zeros otherwise, and for a lane without an entry).
struct PlaneRec { float4 e0, e1, e2; };
template <bool COORD>
__device__ __forceinline__ PlaneRec gather_planes(const float4* splat_b, const uint2 rec) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  PlaneRec p = {z, z, z};
  if constexpr (COORD) {
    // loaded unconditionally (an idle lane reads record 0) and zeroed by selects: loads under a branch reach the staging code through a
    // PHI that the register allocator parks in scratch -- a store, a full wait and a load per round
    const bool live = rec.y != kNoPos;
    const float4* sb = splat_b + 3 * (size_t)(live ? rec.x : 0u);
    const float4 t0 = sb[0], t1 = sb[1], t2 = sb[2];
    p.e0 = live ? t0 : z; p.e1 = live ? t1 : z; p.e2 = live ? t2 : z;
  }
  return p;
}

// ================================================================================ forward ==
// Every round gathers its own records first and relies on the other waves of the SIMD to cover the latency (a software pipeline
// through registers -- the records of round r+1 gathered while round r is blended -- costs ~20 VGPRs and measured 1-2 % slower).
#ifndef RADEGS_FWD_WAVES
#define RADEGS_FWD_WAVES 7   // waves per SIMD the register allocator must leave room for in depth mode (72 VGPRs; left alone it takes 74 = 6 waves:
                             // same-box A/B 0.308 against 0.320 ms; a budget of 64 = 8 waves spills and gains nothing)
#endif
template <bool COORD, bool DEPTH>
__global__ void __launch_bounds__(64, COORD ? 1 : RADEGS_FWD_WAVES) blend_fwd_streams_kernel(const BlendFwdArgs a) {
  constexpr bool NORMAL = COORD || DEPTH;
  __shared__ float4 lds_a[4 * kGrpSlots * 4];
  __shared__ float4 lds_b[COORD ? 4 * kGrpSlots * 3 : 1];
  __shared__ uint32_t lds_con[4 * 16];   // the staged entries' contributor numbers (position in the tile list + 1)

  const int item = xcd_band_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x, grp = lane >> 4, l = lane & 15;
  const StreamRow geo = stream_row_geometry(a.blk_order, item, grp, l, a.gx);
  const uint32_t bid = geo.bid;
  const int tile = geo.tile, blk = geo.blk, px = geo.px, py0 = geo.py0;
  const int W = a.W, H = a.H;
  const float pixfx = (float)px;

  const uint2 range = a.ranges[tile];
  const uint32_t n_tile = range.y - range.x;
  uint32_t n_g = n_tile ? a.blk_count[(size_t)tile * kBlocksPerTile + blk] : 0u;   // uniform inside the row
  uint32_t* chunks = a.blk_chunks + (size_t)a.blk_base[bid] * kChunkWords;

  // Tw: the pixel's transmittance while it is alive.  The entry that terminates it (forward.cu:570-573: T(1-alpha) < 1e-4) is applied to
  // Tw all the same -- Tw only falls, so every later candidate then fails T(1-alpha) >= 1e-4 by itself: "done" needs no flag and the
  // update is ONE select on `ok` (rounds 2-5 kept the final T in Tw with its sign flipped: two selects per pixel and pair).  The final T
  // the epilogue needs (the background term only) is 1 - sum(alpha T) = 1 - out_alpha, as the backward takes it (backward.cu:668).
  float pixfy[2], Tw[2], Cr[2], Cg[2], Cb[2], weight[2];
  float Dep[2], mDep[2], Nx[2], Ny[2], Nz[2];
  float Co[COORD ? 2 : 1][3], mCo[COORD ? 2 : 1][3];
  uint32_t last_c[2], max_c[2];
  bool inside[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int py = py0 + kStreamRowStep * s;
    pixfy[s] = (float)py;
    inside[s] = px < W && py < H;
    Tw[s] = inside[s] ? 1.0f : 0.0f; Cr[s] = Cg[s] = Cb[s] = 0.f; weight[s] = 0.f;
    Dep[s] = mDep[s] = 0.f; Nx[s] = Ny[s] = Nz[s] = 0.f;
    last_c[s] = 0; max_c[s] = 0xFFFFFFFFu;
    if constexpr (COORD) {
#pragma unroll
      for (int c = 0; c < 3; c++) { Co[s][c] = 0.f; mCo[s][c] = 0.f; }
    }
  }
  {  // a row whose pixels are all outside the image consumes nothing
    const uint64_t bal = __ballot(Tw[0] < 0.0001f && Tw[1] < 0.0001f);
    if (((bal >> (grp * 16)) & 0xFFFFull) == 0xFFFFull) n_g = 0u;
  }

  uint32_t nmax = row_uniform_max(n_g);
  const int goff = grp * kGrpSlots;

  for (uint32_t r = 0; r * 16u < nmax; r++) {
    const uint2 rec = load_list_word(chunks, r, l, n_g);
    const PlaneRec pl = gather_planes<COORD>(a.splat_b, rec);
    __syncthreads();   // (one wave per workgroup: orders this round's LDS writes after the previous round's reads)
    gather_rows_to_lds(a.splat_a, rec.y != kNoPos ? rec.x : kNoId, lane, lds_a, kGrpSlots * 4);
    lds_con[grp * 16 + l] = rec.y + 1u;
    if constexpr (COORD) { lds_b[(goff + l) * 3 + 0] = pl.e0; lds_b[(goff + l) * 3 + 1] = pl.e1; lds_b[(goff + l) * 3 + 2] = pl.e2; }
    __syncthreads();
    const int cnt = (int)min(16u, n_g - min(n_g, r * 16u));   // live entries of this row in this round
    const int trip = __builtin_amdgcn_readfirstlane((int)min(16u, nmax - r * 16u));   // wave-uniform, and on the scalar unit: the loop test costs no VALU slot
    uint32_t hist = 0u;        // "this lane's pixel s blended entry j of the round" at bit j + 16 s: the word the backward replays
    // T only falls: once no pixel of the wave is above 0.5 at the start of a round, none of the round's entries can be anybody's
    // median contributor (forward.cu:590-606) -- the median bookkeeping sits behind a wave-uniform branch such rounds do not take
    const bool med_round = NORMAL && __ballot(Tw[0] > 0.5f || Tw[1] > 0.5f) != 0ull;
    for (int j = 0; j < trip; j++) {
      const float4 A = lds_a[(goff + j) * 4 + 0], B = lds_a[(goff + j) * 4 + 1];   // {mx,my,cx,cy} {cz,op,thr (unused here),ts}
      const float4 C = lds_a[(goff + j) * 4 + 2], Dq = lds_a[(goff + j) * 4 + 3];  // {r,g,b,rpx} {rpy,nx,ny,nz}
      float4 E0, E1, E2;
      if constexpr (COORD) { E0 = lds_b[(goff + j) * 3 + 0]; E1 = lds_b[(goff + j) * 3 + 1]; E2 = lds_b[(goff + j) * 3 + 2]; }
      const float dx = A.x - pixfx;
      const float a_x = (A.z * dx) * dx;
      const float b_xy = A.w * dx;
      const float t_dx = DEPTH ? fmaf(C.w, dx, B.w) : 0.f;   // the depth plane at (dx, .): the "dx" half once for the lane's two pixels
      float t_new[2], t_dep[2];
      bool okk[2], actt[2];
#pragma unroll
      for (int s = 0; s < 2; s++) {
        // the decision chain of forward.cu:552-573, one rounding per operation (rg_blend.h)
        // (the two pixels' chains as ONE chain of packed fp32 instructions -- v_pk_mul / add / fma, the same roundings component-wise, 18
        // instructions fewer per step -- measured +10 % on the same box: 0.350-0.363 against 0.321-0.324 ms; two interleaved scalar chains it is)
        const float dy = A.y - pixfy[s];
        const float power = splat_power(a_x, b_xy, B.x, dy);
        const float G = exp_spec_floor(power);   // == exp_spec(power) wherever alpha can reach 1/255
        const float alpha = fminf(0.99f, B.y * G);
        const float test_T = Tw[s] * (1 - alpha);
        const bool ok = !(power > 0.0f) && !(alpha < 1.0f / 255.0f);   // (a slot past the row's list holds an all-zero record: alpha = 0)
        const bool act = ok && !(test_T < 0.0001f);
        // The accumulation runs under the pair's own lane mask: no select of 0 for the weight, one OR for the contribution bit -- five
        // instructions fewer per round step than the select form (same-box A/B: 0.312 against 0.330 ms).  Putting the transmittance update
        // and the median terms under nested masks as well measured no better than the select form (the extra branches).
        float t_here = 0.f;
        if constexpr (DEPTH) t_here = fmaf(Dq.x, dy, t_dx);
        t_dep[s] = t_here;
        if (act) {
          const float aT = alpha * Tw[s];
          Cr[s] = fmaf(C.x, aT, Cr[s]); Cg[s] = fmaf(C.y, aT, Cg[s]); Cb[s] = fmaf(C.z, aT, Cb[s]);
          if constexpr (COORD) {
            float c[3];
            coord_planes(E0, E1, E2, dx, dy, c);
            Co[s][0] = fmaf(c[0], aT, Co[s][0]); Co[s][1] = fmaf(c[1], aT, Co[s][1]); Co[s][2] = fmaf(c[2], aT, Co[s][2]);
          }
          if constexpr (DEPTH) Dep[s] = fmaf(t_here, aT, Dep[s]);
          if constexpr (NORMAL) { Nx[s] = fmaf(Dq.y, aT, Nx[s]); Ny[s] = fmaf(Dq.z, aT, Ny[s]); Nz[s] = fmaf(Dq.w, aT, Nz[s]); }
          weight[s] += aT;
          hist |= (s ? 0x10000u : 1u) << j;
        }
        t_new[s] = test_T; okk[s] = ok; actt[s] = act;
      }
      if (med_round) {   // Tw still holds the transmittance BEFORE this entry
        const uint32_t contributor = lds_con[grp * 16 + j];
#pragma unroll
        for (int s = 0; s < 2; s++) {
          const bool med = actt[s] && (Tw[s] > 0.5f);
          if constexpr (COORD) {
            const float dy = A.y - pixfy[s];
            float c[3];
            coord_planes(E0, E1, E2, dx, dy, c);
            mCo[s][0] = med ? c[0] : mCo[s][0]; mCo[s][1] = med ? c[1] : mCo[s][1]; mCo[s][2] = med ? c[2] : mCo[s][2];
          }
          if constexpr (DEPTH) mDep[s] = med ? t_dep[s] : mDep[s];
          max_c[s] = med ? contributor : max_c[s];
        }
      }
#pragma unroll
      for (int s = 0; s < 2; s++) Tw[s] = okk[s] ? t_new[s] : Tw[s];   // ok && !act: the pixel terminates here (forward.cu:570-573) -- see Tw above
    }
    if (cnt > 0) chunks[(size_t)r * kChunkWords + 32 + l] = hist;
    // last contributor (forward.cu:625): the round's highest blended entry, its number read back once per round
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const uint32_t hs = (hist >> (16 * s)) & 0xFFFFu;
      if (hs) last_c[s] = lds_con[grp * 16 + (31 - __builtin_clz(hs))];
    }
    // rows whose pixels have all terminated stop consuming their list
    const uint64_t bal = __ballot(Tw[0] < 0.0001f && Tw[1] < 0.0001f);   // below 1e-4 nothing can blend any more
    if (((bal >> (grp * 16)) & 0xFFFFull) == 0xFFFFull) n_g = min(n_g, (r + 1u) * 16u);
    nmax = row_uniform_max(n_g);
  }
  if (l == 0 && n_tile) a.blk_consumed[(size_t)tile * kBlocksPerTile + blk] = n_g;

  // ---- epilogue ----
#pragma unroll
  for (int s = 0; s < 2; s++) {
    if (!inside[s]) continue;
    // final transmittance: 1 - weight[s] (see Tw above; the tile-wide kernel keeps the running product and passes that: radegs_kernels.hip)
    blend_fwd_epilogue<COORD, DEPTH>(a, px, py0 + kStreamRowStep * s, 1.0f - weight[s], last_c[s], max_c[s], Cr[s], Cg[s], Cb[s], weight[s],
                                     Co[COORD ? s : 0], mCo[COORD ? s : 0], Dep[s], mDep[s], Nx[s], Ny[s], Nz[s]);
  }
}

// =============================================================================== backward ==
// Same mathematics as blend_bwd_packed_kernel (one "behind" accumulator Q per pixel, alpha = 0 turns a pixel's whole update
// into an exact no-op); what differs is where the decisions come from (the forward's contribution bits) and that nothing in
// the loop is conditional.

// What the blend backwards leave in the accumulator record (SplatAcc order, 16 | 32 floats).  Components 9..14 are RAW MOMENTS of
// h = opacity G dL/dalpha about the Gaussian's own centre, not the reference's sums: the mean2D / conic gradients are linear in them with
// per-Gaussian coefficients (backward.cu:981-1012), so those products are taken ONCE per Gaussian by preprocess_bwd (rg_preprocess_bwd.h:
// SplatAcc::raw -- from the conic and the planes it re-derives anyway: no extra read) instead of once per (pixel, entry) pair here:
//    [9]  sum h dx           dL_dmean2D.x = -(cx [9] + cy [10]) + rpx [3] (+ sum_c cp_c.x [16 + c])
//    [10] sum h dy           dL_dmean2D.y = -(cy [9] + cz [10]) + rpy [3] (+ sum_c cp_c.y [16 + c])
//    [11] sum |h| (|ex| W/2 + |ey| H/2)      the abs-gradient as it is   (ex, ey: the conic applied to (dx, dy))
//    [12] sum h dx dx        dL_dconic.x = -1/2 [12]
//    [13] sum h dx dy        dL_dconic.y = -1/2 [13]
//    [14] sum h dy dy        dL_dconic.w = -1/2 [14]
//    [15] sum u              (u = G dL/dalpha: the opacity gradient, as before)
// (dx, dy are relative to the Gaussian's own mean, so the moments add up across blocks and tiles without cancellation.)  The two
// pixels of a lane share dx: everything that is "times dx" is applied once per lane to the two pixels' sum.
#ifndef RADEGS_BWD_WAVES
#define RADEGS_BWD_WAVES 5   // waves per SIMD the register allocator leaves room for (same-box A/B: 6 -> 0.545 ms with a spill, 5 -> 0.535)
#endif
template <bool COORD, bool DEPTH>
__global__ void __launch_bounds__(64, COORD ? 3 : RADEGS_BWD_WAVES) blend_bwd_streams_kernel(const BlendBwdArgs a) {
  constexpr bool NORMAL = COORD || DEPTH;
  constexpr int REC = COORD ? 32 : 16;
  constexpr int RW = 4;   // 16-byte rows per staged record
  // The image state must hold the entry streams of the forward it came from (ImageState::stream_tag): replaying anything else would
  // produce silently wrong gradients.  A buffer without them is a contract violation of the caller (the host-side registry only hands
  // this kernel buffers a stream forward wrote; rg_launch.inc): raise the flag in the host's mapped error word AND poison the
  // accumulator, so that this very backward returns NaN gradients (the flag itself only surfaces on the next call into the library;
  // ADVICE r5); the device context survives.
  if (a.stream_tag[0] != kStreamTag) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && a.stream_err) __hip_atomic_store(a.stream_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const size_t n = (size_t)a.P * REC;
    for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < n; i += (size_t)gridDim.x * 64) a.acc[i] = __builtin_nanf("");
    return;
  }
  // a row's 16 staged records + ONE 16-byte pad: the four rows read slot j in lockstep, the pad puts them four banks apart (a whole
  // pad slot per row, as in the forward, would cost the 24th wave of a CU its LDS)
  constexpr int kRowV4 = 16 * RW + 1;
  __shared__ v4f lds_a[4 * kRowV4];
  __shared__ uint32_t lds_pos[4 * 16];
  __shared__ uint32_t lds_id[4 * 16];
  __shared__ v4f lds_b[COORD ? 4 * kGrpSlots * 3 : 1];
  __shared__ __attribute__((aligned(16))) float lds_red[4 * kRedRowFloats];

  const int item = xcd_band_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x, grp = lane >> 4, l = lane & 15;
  const StreamRow geo = stream_row_geometry(a.blk_order, item, grp, l, a.gx);
  const uint32_t bid = geo.bid;
  const int tile = geo.tile, blk = geo.blk, px = geo.px, py0 = geo.py0;
  const int W = a.W, H = a.H;
  const float pixfx = (float)px;
  const uint2 range = a.ranges[tile];
  const uint32_t n_tile = range.y - range.x;
  const uint32_t n_c = n_tile ? a.blk_consumed[(size_t)tile * kBlocksPerTile + blk] : 0u;
  const uint32_t* chunks = a.blk_chunks + (size_t)a.blk_base[bid] * kChunkWords;
  const uint32_t nmax = row_uniform_max(n_c);
  if (nmax == 0u) return;
  const RowReduceAddr red = row_reduce_addr(lds_red, grp, l);

  // ---- per-pixel prologue ----
  float pixfy[2], T[2], Q[2], dLa[2], tb[2], dLc[2][3], dLt[2], dLmt[2], dLn[2][3];
  float dLco[COORD ? 2 : 1][3], dLmco[COORD ? 2 : 1][3];
  uint32_t max_cm1[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int py = py0 + kStreamRowStep * s;
    pixfy[s] = (float)py;
    const PixelCotangents ct = pixel_cotangents<COORD, DEPTH>(a, px, py);
    T[s] = ct.T; Q[s] = 0.f; dLa[s] = ct.dLa; tb[s] = ct.tb;
    dLt[s] = ct.dLt; dLmt[s] = ct.dLmt;
    max_cm1[s] = ct.max_cm1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      dLc[s][c] = ct.dLc[c]; dLn[s][c] = ct.dLn[c];
      if constexpr (COORD) { dLco[s][c] = ct.dLco[c]; dLmco[s][c] = ct.dLmco[c]; }
    }
  }
  const float cW = 0.5f * W, cH = 0.5f * H;

  const int rtop = (int)((nmax + 15u) >> 4) - 1;
  auto load_hist = [&](int r) { return (r >= 0 && (uint32_t)r * 16u < n_c) ? chunks[(size_t)r * kChunkWords + 32 + l] : 0u; };
  const int goff = grp * kGrpSlots;
  constexpr float kLog2e = 1.44269504088896341f;

  // The NEXT round's list words (Gaussian id, position, contribution bits) are requested one round ahead, so that a round starts with
  // ONE memory latency (the record gather) instead of two dependent ones: behind the atomics' backlog in the memory pipe a load takes
  // its time (same-box A/B: 0.535 -> 0.524 ms; prefetching the records too costs 16 registers and loses: 0.557).
  uint2 rec_nxt = load_list_word(chunks, (uint32_t)rtop, l, n_c);
  uint32_t hist_nxt = load_hist(rtop);
  for (int r = rtop; r >= 0; r--) {
    const uint2 rec_cur = rec_nxt;
    const PlaneRec pl = gather_planes<COORD>(a.splat_b, rec_cur);
    const uint32_t hist = hist_nxt;
    rec_nxt = load_list_word(chunks, (uint32_t)(r - 1), l, n_c); hist_nxt = load_hist(r - 1);
    __syncthreads();
    {  // stage the records as they lie in memory -- {mx,my,cx,cy} {cz,op,thr,ts} {r,g,b,rpx} {rpy,nx,ny,nz} -- four lanes per record
       // (gather_rows_to_lds), and next to them the entries' Gaussian ids and positions in the tile list
      gather_rows_to_lds(a.splat_a, rec_cur.y != kNoPos ? rec_cur.x : kNoId, lane, lds_a, kRowV4);
      lds_pos[grp * 16 + l] = rec_cur.y;
      lds_id[grp * 16 + l] = rec_cur.x;
      if constexpr (COORD) {
        const float4 e0 = pl.e0, e1 = pl.e1, e2 = pl.e2;
        lds_b[(goff + l) * 3 + 0] = v4f{e0.x, e0.y, e0.z, e0.w}; lds_b[(goff + l) * 3 + 1] = v4f{e1.x, e1.y, e1.z, e1.w};
        lds_b[(goff + l) * 3 + 2] = v4f{e2.x, e2.y, e2.z, e2.w};
      }
    }
    __syncthreads();
    const int trip = (int)min(16u, nmax - (uint32_t)r * 16u);   // wave-uniform
    // Does any pixel of the wave have its median contributor (forward.cu:590-606: the last entry blended while T > 0.5) among this
    // round's entries?  A pixel has exactly one, mostly near the front of its list: the median terms of the sums sit behind a
    // wave-uniform branch that most rounds do not take.
    bool med_round;
    {
      const uint32_t live = min(16u, n_c - min(n_c, (uint32_t)r * 16u));   // valid entries of this row in this round
      const uint32_t p_lo = lds_pos[grp * 16], p_hi = lds_pos[grp * 16 + (live ? live - 1u : 0u)];
      const bool m = live != 0u && ((max_cm1[0] - p_lo <= p_hi - p_lo) || (max_cm1[1] - p_lo <= p_hi - p_lo));
      med_round = __ballot(m) != 0ull;
    }
    for (int j = trip - 1; j >= 0; j--) {
      const v4f* rp = lds_a + grp * kRowV4 + j * RW;
      const v4f A = rp[0], R1 = rp[1], R2 = rp[2], R3 = rp[3];
      // the loop's names for the fields (register renaming only): B {cz, op, ts, rpx}, C {rpy, r, g, b}, Dq {nx, ny, nz, -}
      const v4f B = v4f{R1.x, R1.y, R1.w, R2.w}, C = v4f{R3.x, R2.x, R2.y, R2.z}, Dq = v4f{R3.y, R3.z, R3.w, 0.f};
      v4f E0, E1, E2;
      if constexpr (COORD) { E0 = lds_b[(goff + j) * 3 + 0]; E1 = lds_b[(goff + j) * 3 + 1]; E2 = lds_b[(goff + j) * 3 + 2]; }
      const uint32_t gid = lds_id[grp * 16 + j];
      const float dx = A.x - pixfx;
      const float a_x = (A.z * dx) * dx, b_xy = A.w * dx;   // the forward's association of `power`
      const float dxcx = dx * A.z;
      const float tx = fmaf(B.w, dx, B.z);              // ts + rpx dx
      // the lane's sums over its two pixels
      float s_col[3], s_nrm[3], s_dt = 0.f, s_dty = 0.f, s_u = 0.f, s_h = 0.f, s_hy = 0.f, s_hyy = 0.f, s_ab = 0.f;
      float s_co[COORD ? 3 : 1], s_coy[COORD ? 3 : 1];
      int any_keep = 0;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const float dy = A.y - pixfy[s];
        // `power` in the forward's (= the reference's) order of operations, one rounding each: a needle-thin splat's quadratic
        // form is a difference of terms thousands of times its value, and any other association moves exp(power) by per cent
        const float pw = kLog2e * splat_power(a_x, b_xy, B.x, dy);
        // the forward's decision for this (pixel, entry) as an all-ones / all-zeros word: ANDed onto the bits of the exponential
        // it switches the pair off exactly (alpha = 0, G = 0) whatever exp2 returned (an indefinite conic may overflow it)
        const int keep = __builtin_amdgcn_sbfe((int)hist, (unsigned)(j + 16 * s), 1u);
        any_keep |= keep;
        const float G = __int_as_float(__float_as_int(__builtin_amdgcn_exp2f(pw)) & keep);
        const float alpha = fminf(0.99f, B.y * G);
        const float inv1ma = rcp_refined(1.f - alpha);
        T[s] = T[s] * inv1ma;
        const float dch = alpha * T[s];
        // V = <cotangent of this pixel, blended quantities of this Gaussian>
        float V = dLa[s];
        V = fmaf(C.y, dLc[s][0], V); V = fmaf(C.z, dLc[s][1], V); V = fmaf(C.w, dLc[s][2], V);
        float dco[3], dt_ = 0.f;
        if constexpr (COORD) {
          float cc[3];
          coord_planes(E0, E1, E2, dx, dy, cc);
#pragma unroll
          for (int c = 0; c < 3; c++) {
            V = fmaf(cc[c], dLco[s][c], V);
            dco[c] = dch * dLco[s][c];
          }
        }
        if constexpr (DEPTH) {
          const float t = fmaf(C.x, dy, tx);
          V = fmaf(t, dLt[s], V);
          dt_ = dch * dLt[s];
        }
        if constexpr (NORMAL) { V = fmaf(Dq.x, dLn[s][0], V); V = fmaf(Dq.y, dLn[s][1], V); V = fmaf(Dq.z, dLn[s][2], V); }
        const float dop = V - Q[s];
        Q[s] = fmaf(alpha, dop, Q[s]);
        const float wq = fmaf(dop, T[s], inv1ma * tb[s]);
        const float u = G * wq;
        const float hq = B.y * u;          // h = opacity * u: the moments below are h's, so that nobody needs the opacity again
        const float hy = hq * dy;
        const float ex = fmaf(dy, A.w, dxcx), ey = fmaf(dy, B.x, b_xy);   // the conic applied to (dx, dy)
        const float tt = fmaf(fabsf(ey), cH, fabsf(ex) * cW);
        if (s == 0) {
          s_col[0] = dch * dLc[s][0]; s_col[1] = dch * dLc[s][1]; s_col[2] = dch * dLc[s][2];
          if constexpr (NORMAL) { s_nrm[0] = dch * dLn[s][0]; s_nrm[1] = dch * dLn[s][1]; s_nrm[2] = dch * dLn[s][2]; }
          if constexpr (DEPTH) { s_dt = dt_; s_dty = dt_ * dy; }
          s_u = u; s_h = hq; s_hy = hy; s_hyy = hy * dy; s_ab = fabsf(hq) * tt;
          if constexpr (COORD) {
#pragma unroll
            for (int c = 0; c < 3; c++) { s_co[c] = dco[c]; s_coy[c] = dco[c] * dy; }
          }
        } else {
          s_col[0] = fmaf(dch, dLc[s][0], s_col[0]); s_col[1] = fmaf(dch, dLc[s][1], s_col[1]); s_col[2] = fmaf(dch, dLc[s][2], s_col[2]);
          if constexpr (NORMAL) {
            s_nrm[0] = fmaf(dch, dLn[s][0], s_nrm[0]); s_nrm[1] = fmaf(dch, dLn[s][1], s_nrm[1]); s_nrm[2] = fmaf(dch, dLn[s][2], s_nrm[2]);
          }
          if constexpr (DEPTH) { s_dt += dt_; s_dty = fmaf(dt_, dy, s_dty); }
          s_u += u; s_h += hq; s_hy += hy; s_hyy = fmaf(hy, dy, s_hyy); s_ab = fmaf(fabsf(hq), tt, s_ab);
          if constexpr (COORD) {
#pragma unroll
            for (int c = 0; c < 3; c++) { s_co[c] += dco[c]; s_coy[c] = fmaf(dco[c], dy, s_coy[c]); }
          }
        }
      }
      const uint64_t cm = __ballot(any_keep != 0);
      if (cm == 0) continue;
      if (NORMAL && med_round) {   // the median maps' cotangents go to the one entry that is the pixel's median contributor
        const uint32_t pos = lds_pos[grp * 16 + j];
#pragma unroll
        for (int s = 0; s < 2; s++) {
          const bool med = pos == max_cm1[s];
          const float dy = A.y - pixfy[s];
          if constexpr (DEPTH) {
            const float m = med ? dLmt[s] : 0.f;
            s_dt += m; s_dty = fmaf(m, dy, s_dty);
          }
          if constexpr (COORD) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
              const float m = med ? dLmco[s][c] : 0.f;
              s_co[c] += m; s_coy[c] = fmaf(m, dy, s_coy[c]);
            }
          }
        }
      }
      float gv[REC];
      gv[0] = s_col[0]; gv[1] = s_col[1]; gv[2] = s_col[2];
      gv[3] = s_dt; gv[4] = s_dt * dx; gv[5] = s_dty;
      if constexpr (NORMAL) { gv[6] = s_nrm[0]; gv[7] = s_nrm[1]; gv[8] = s_nrm[2]; } else { gv[6] = 0.f; gv[7] = 0.f; gv[8] = 0.f; }
      const float s_hx = s_h * dx;
      gv[9] = s_hx; gv[10] = s_hy; gv[11] = s_ab;
      gv[12] = s_hx * dx; gv[13] = s_hy * dx; gv[14] = s_hyy; gv[15] = s_u;
      if constexpr (COORD) {
#pragma unroll
        for (int c = 0; c < 3; c++) { gv[16 + c] = s_co[c]; gv[19 + 2 * c] = s_co[c] * dx; gv[20 + 2 * c] = s_coy[c]; }
#pragma unroll
        for (int c = 25; c < 32; c++) gv[c] = 0.f;
      }
      // lane l ends with the row total of component l (and of component 16 + l)
      const float tot0 = row_reduce16(*reinterpret_cast<float (*)[16]>(gv), red);
      float tot1 = 0.f;
      if constexpr (REC == 32) tot1 = row_reduce16(*reinterpret_cast<float (*)[16]>(gv + 16), red);
#ifdef RADEGS_EXP_NOATOMIC   // timing experiment: what the loop costs without the memory-side atomic unit (results are wrong)
      if (tot0 == 123.456f && tot1 == 654.321f)
#else
      // the rows with a contributing pixel, as a lane mask put together on the scalar unit and handed to EXEC as it is (three VALU
      // instructions per round step when every lane tests its own row's 16 bits of `cm`)
      uint64_t rows = 0ull;
#pragma unroll
      for (int k = 0; k < 4; k++) rows |= ((cm >> (16 * k)) & 0xFFFFull) ? (0xFFFFull << (16 * k)) : 0ull;
      if (__builtin_amdgcn_inverse_ballot_w64(rows))
#endif
      {   // one 64-byte line per atomic instruction; the record's byte offset in 32 bits next to the scalar base (no 64-bit shift and
          // add per round step): the launcher hands this kernel accumulators below 4 GB only (rg_launch.inc: kStreamBwdMaxAccBytes)
        float* rec = reinterpret_cast<float*>(reinterpret_cast<char*>(a.acc) + (gid * (uint32_t)(REC * 4) + (uint32_t)l * 4u));
        unsafeAtomicAdd(rec, tot0);
        if constexpr (REC == 32) { if (l < 9) unsafeAtomicAdd(rec + 16, tot1); }
      }
    }
  }
}

}  // namespace rg
