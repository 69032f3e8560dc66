// radegs_evalio.hip -- evaluation from files: the step from the files on disk to the tensors the evaluation units take.
//     o3d.io.read_point_cloud / trimesh.load                geometry PLY -> float64 / int64      unpack_points_kernel, unpack_faces_kernel
//     registration.py:66-110 trajectory_alignment           RANSAC over paired camera centres    ransac_eval_kernel -> ransac_select_kernel
//
// The specification is include/radegs.h, "Evaluation from files"; tests/evalio_restatement.py restates it in NumPy.  Built with the default
// FLAGS: -ffp-contract=off, IEEE divide and sqrt -- one rounding per operation in the order written, so the per-pair decisions d < max_dist
// are those of the restatement wherever it keeps its margin.  The only atomics are integer ones (the count of refused face records); the
// best hypothesis is chosen by comparing keys, so every output is repeatable bit for bit and independent of the launch geometry.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_workspace.h"

namespace rgev {

constexpr int kTile = 64;        // records per workgroup of the unpack kernels: at most 64 * 768 B = 48 KB of LDS
constexpr int kThreads = 256;
constexpr int kChunk = RADEGS_EVALIO_RANSAC_CHUNK;
constexpr int kSweeps = RADEGS_EVALIO_RANSAC_SWEEPS;   // one-sided Jacobi on a 3x3 converges quadratically; 8 sweeps leave nothing above rounding, and a fixed count keeps a wave together

// ------------------------------------------------------------------- records -> values -------------------------------------------------------------------
__host__ __device__ inline int type_size(int t) { return (unsigned)t < 8u ? (int)((0x84442211u >> (4 * t)) & 15u) : 0; }

__device__ __forceinline__ uint32_t bytes4(const uint32_t* lds, int a) {       // the 4 bytes at byte address a, any alignment
  const int q = a >> 2;
  const uint64_t two = ((uint64_t)lds[q + 1] << 32) | lds[q];
  return (uint32_t)(two >> (8 * (a & 3)));
}

// The tile's records, from byte `begin` of the buffer, as an LDS image that starts on the dword holding that byte.  Returns the byte within the
// image at which the first record starts.  Three zero words follow the image: bytes4's second word, and the same for the high half of an f8.
__device__ __forceinline__ int stage_records(uint32_t* img, const uint32_t* __restrict__ buffer, long long begin, int nbytes) {
  const int shift = (int)(begin & 3);
  const int words = (shift + nbytes + 3) >> 2;
  const uint32_t* src = buffer + (begin >> 2);
  for (int i = threadIdx.x; i < words; i += kThreads) img[i] = src[i];
  if (threadIdx.x < 3) img[words + threadIdx.x] = 0;
  return shift;
}

__device__ __forceinline__ long long load_integer(const uint32_t* img, int a, int type) {
  const uint32_t lo = bytes4(img, a);
  switch (type) {
    case RADEGS_MODELIO_I1: return (long long)(int8_t)lo;
    case RADEGS_MODELIO_U1: return (long long)(uint8_t)lo;
    case RADEGS_MODELIO_I2: return (long long)(int16_t)lo;
    case RADEGS_MODELIO_U2: return (long long)(uint16_t)lo;
    case RADEGS_MODELIO_I4: return (long long)(int32_t)lo;
    default: return (long long)lo;   // U4
  }
}

struct PointColumns {
  int offset[3], type[3];
};

// 192 lanes of a workgroup take the 64 x 3 values of its tile: consecutive lanes store consecutive doubles
__global__ void __launch_bounds__(kThreads) unpack_points_kernel(long long N, int S, const uint32_t* __restrict__ buffer, long long byte_offset, PointColumns c,
                                                                 double* __restrict__ out) {
  extern __shared__ __align__(16) uint32_t img[];
  const long long row0 = (long long)blockIdx.x * kTile;
  const int n = (int)min((long long)kTile, N - row0);
  const int shift = stage_records(img, buffer, byte_offset + row0 * S, n * S);
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= 3 * n) return;
  const int r = t / 3, k = t - 3 * r;
  const int a = shift + r * S + c.offset[k], type = c.type[k];
  double v;
  if (type == RADEGS_MODELIO_F8)
    v = __longlong_as_double((long long)(((uint64_t)bytes4(img, a + 4) << 32) | bytes4(img, a)));   // the bits as they are
  else if (type == RADEGS_MODELIO_F4)
    v = (double)__uint_as_float(bytes4(img, a));                                                    // exact
  else
    v = (double)load_integer(img, a, type);                                                         // exact: at most 32 bits
  out[3 * row0 + t] = v;
}

// 192 lanes take the 64 x 3 indices; a record is refused (counted) when its list length is not 3 or an index is outside [0, V)
__global__ void __launch_bounds__(kThreads) unpack_faces_kernel(long long F, int S, const uint32_t* __restrict__ buffer, long long byte_offset, int count_offset,
                                                                int count_type, int index_offset, int index_type, long long V,
                                                                long long* __restrict__ faces, unsigned int* __restrict__ bad) {
  extern __shared__ __align__(16) uint32_t img[];
  __shared__ int bad_row[kTile];
  __shared__ unsigned int bad_rows;
  const long long row0 = (long long)blockIdx.x * kTile;
  const int n = (int)min((long long)kTile, F - row0);
  const int shift = stage_records(img, buffer, byte_offset + row0 * S, n * S);
  const int t = threadIdx.x;
  if (t < kTile) bad_row[t] = 0;
  if (t == 0) bad_rows = 0u;
  __syncthreads();
  if (t < 3 * n) {
    const int r = t / 3, k = t - 3 * r;
    const int a = shift + r * S;
    const long long count = load_integer(img, a + count_offset, count_type);
    const long long index = load_integer(img, a + index_offset + 4 * k, index_type);
    faces[3 * row0 + t] = index;
    if (count != 3 || index < 0 || index >= V) bad_row[r] = 1;   // several lanes may write the same 1
  }
  __syncthreads();
  if (t < n && bad_row[t]) atomicAdd(&bad_rows, 1u);
  __syncthreads();
  if (t == 0 && bad_rows) atomicAdd(bad, bad_rows);
}

// ------------------------------------------------------------------- correspondence RANSAC -------------------------------------------------------------------
// the generator of include/radegs.h: a function of (seed, h, draw) alone
__host__ __device__ inline uint32_t draw_u32(unsigned long long seed, unsigned long long h, unsigned long long k) {
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull + h * 0xD1B54A32D192ED03ull + k * 0x8CB92BA72F3D8DD7ull + 0x2545F4914F6CDD1Dull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

// `n` distinct indices of [0, N) in draw order: draw k picks the r-th index not yet taken, r = (u (N - k)) >> 32
__device__ __forceinline__ void draw_sample(unsigned long long seed, unsigned long long h, int n, uint32_t N, uint32_t* sample) {
  uint32_t taken[RADEGS_EVALIO_RANSAC_MAX_N];   // ascending
#pragma unroll
  for (int k = 0; k < RADEGS_EVALIO_RANSAC_MAX_N; k++) {
    if (k >= n) break;
    uint32_t r = (uint32_t)(((unsigned long long)draw_u32(seed, h, (unsigned long long)k) * (unsigned long long)(N - (uint32_t)k)) >> 32);
#pragma unroll
    for (int j = 0; j < RADEGS_EVALIO_RANSAC_MAX_N; j++)
      if (j < k && r >= taken[j]) r++;
    sample[k] = r;
    uint32_t carry = r;                          // insert r, keeping `taken` ascending
#pragma unroll
    for (int j = 0; j < RADEGS_EVALIO_RANSAC_MAX_N; j++) {
      if (j < k && taken[j] > carry) {
        const uint32_t tmp = taken[j];
        taken[j] = carry;
        carry = tmp;
      }
    }
    taken[k] = carry;
  }
}

// one rotation of the one-sided Jacobi method: makes columns p and q of A orthogonal, and applies the same rotation to V
__device__ __forceinline__ void rotate(double (&A)[3][3], double (&V)[3][3], int p, int q) {
  const double alpha = (A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p];
  const double beta = (A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q];
  const double gamma = (A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q];
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  if (gamma == 0.0 || !(zeta == zeta)) {   // already orthogonal (0 / 0 included)
    c = 1.0;
    s = 0.0;
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double ap = A[r][p], aq = A[r][q], vp = V[r][p], vq = V[r][q];
    A[r][p] = c * ap - s * aq;
    A[r][q] = s * ap + c * aq;
    V[r][p] = c * vp - s * vq;
    V[r][q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ void swap_columns(double (&A)[3][3], double (&V)[3][3], double (&sig)[3], int p, int q) {
  if (sig[p] < sig[q]) {
    double tmp = sig[p]; sig[p] = sig[q]; sig[q] = tmp;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      tmp = A[r][p]; A[r][p] = A[r][q]; A[r][q] = tmp;
      tmp = V[r][p]; V[r][p] = V[r][q]; V[r][q] = tmp;
    }
  }
}

// Eigen's umeyama with scaling for the sample of hypothesis h: T [12] = rows 0-2 of the 4x4.  false: a sample without extent, or a
// transformation that is not finite.
__device__ bool sample_similarity(unsigned long long seed, unsigned long long h, int n, uint32_t N, const double* __restrict__ source,
                                  const double* __restrict__ target, double* T) {
  uint32_t sample[RADEGS_EVALIO_RANSAC_MAX_N];
  draw_sample(seed, h, n, N, sample);
  double ss[3] = {0.0, 0.0, 0.0}, st[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < RADEGS_EVALIO_RANSAC_MAX_N; k++) {
    if (k >= n) break;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      ss[a] += source[3 * (size_t)sample[k] + a];
      st[a] += target[3 * (size_t)sample[k] + a];
    }
  }
  const double cnt = (double)n;
  const double ms[3] = {ss[0] / cnt, ss[1] / cnt, ss[2] / cnt}, mt[3] = {st[0] / cnt, st[1] / cnt, st[2] / cnt};
  double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, var = 0.0;
#pragma unroll
  for (int k = 0; k < RADEGS_EVALIO_RANSAC_MAX_N; k++) {
    if (k >= n) break;
    double ds[3], dt[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      ds[a] = source[3 * (size_t)sample[k] + a] - ms[a];
      dt[a] = target[3 * (size_t)sample[k] + a] - mt[a];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) A[r][c] += dt[r] * ds[c];
    var += (ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2];
  }
  if (!(var > 0.0)) return false;
  var = var / cnt;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) A[r][c] = A[r][c] / cnt;
  // A = U diag(sig) V^T: after the sweeps the columns of A are U diag(sig)
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < kSweeps; sweep++) {
    rotate(A, V, 0, 1);
    rotate(A, V, 0, 2);
    rotate(A, V, 1, 2);
  }
  double sig[3];
#pragma unroll
  for (int c = 0; c < 3; c++) sig[c] = sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
  swap_columns(A, V, sig, 0, 1);
  swap_columns(A, V, sig, 1, 2);
  swap_columns(A, V, sig, 0, 1);
  const double u0[3] = {A[0][0] / sig[0], A[1][0] / sig[0], A[2][0] / sig[0]}, u1[3] = {A[0][1] / sig[1], A[1][1] / sig[1], A[2][1] / sig[1]};
  const double cr[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
  const double det_v = (V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0])) +
                       V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  // the third left vector is +-cr; with S = diag(1, 1, det U det V) the product U S V^T has the column (det V) cr in its place
  const double sv = det_v < 0.0 ? -1.0 : 1.0;
  const double su = ((A[0][2] * cr[0] + A[1][2] * cr[1]) + A[2][2] * cr[2]) < 0.0 ? -1.0 : 1.0;
  const double scale = ((sig[0] + sig[1]) + (su * sv) * sig[2]) / var;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double row[3];
#pragma unroll
    for (int c = 0; c < 3; c++) row[c] = scale * ((u0[r] * V[c][0] + u1[r] * V[c][1]) + (sv * cr[r]) * V[c][2]);
    T[4 * r] = row[0];
    T[4 * r + 1] = row[1];
    T[4 * r + 2] = row[2];
    T[4 * r + 3] = mt[r] - ((row[0] * ms[0] + row[1] * ms[1]) + row[2] * ms[2]);
#pragma unroll
    for (int c = 0; c < 4; c++) ok = ok && isfinite(T[4 * r + c]);
  }
  return ok;
}

// One lane per hypothesis.  The pairs pass through LDS kChunk at a time; every lane reads the same pair: a broadcast, no bank conflict.
__global__ void __launch_bounds__(kThreads) ransac_eval_kernel(uint32_t N, const double* __restrict__ source, const double* __restrict__ target, double max_dist,
                                                               int n, long long K, unsigned long long seed, int* __restrict__ counts,
                                                               double* __restrict__ sumsq) {
  __shared__ __align__(16) double pairs[6 * kChunk];
  const long long h = (long long)blockIdx.x * kThreads + threadIdx.x;
  double T[12];
  const bool live = h < K && sample_similarity(seed, (unsigned long long)h, n, N, source, target, T);
  int count = 0;
  double sum = 0.0;
  for (uint32_t base = 0; base < N; base += kChunk) {
    const int m = (int)min((uint32_t)kChunk, N - base);
    __syncthreads();                                     // the chunk before has been read
    for (int i = threadIdx.x; i < 3 * m; i += kThreads) {
      const int p = i / 3, a = i - 3 * p;
      pairs[6 * p + a] = source[3 * (size_t)base + i];
      pairs[6 * p + 3 + a] = target[3 * (size_t)base + i];
    }
    __syncthreads();
    if (live) {
      for (int p = 0; p < m; p++) {
        const double x = pairs[6 * p], y = pairs[6 * p + 1], z = pairs[6 * p + 2];
        const double dx = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - pairs[6 * p + 3];
        const double dy = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - pairs[6 * p + 4];
        const double dz = (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - pairs[6 * p + 5];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (sqrt(d2) < max_dist) {
          count++;
          sum += d2;
        }
      }
    }
  }
  if (h < K) {
    counts[h] = count;
    sumsq[h] = sum;
  }
}

// better(a, b): more inliers; then the smaller sqrt(sumsq / count); then the smaller h
struct Best {
  int count;
  double rmse;
  long long h;
};
__device__ __forceinline__ bool better(const Best& a, const Best& b) {
  if (a.count != b.count) return a.count > b.count;
  if (a.rmse != b.rmse) return a.rmse < b.rmse;
  return a.h < b.h;
}

// One workgroup: the best hypothesis of counts / sumsq, then its transformation once more.  out [15] = T rows 0-2, count, sumsq, h.
__global__ void __launch_bounds__(kThreads) ransac_select_kernel(uint32_t N, const double* __restrict__ source, const double* __restrict__ target, int n,
                                                                 long long K, unsigned long long seed, const int* __restrict__ counts,
                                                                 const double* __restrict__ sumsq, double* __restrict__ out) {
  __shared__ Best best[kThreads];
  Best mine = {0, 0.0, K};
  for (long long h = threadIdx.x; h < K; h += kThreads) {
    const int c = counts[h];
    if (c <= 0) continue;
    const Best b = {c, sqrt(sumsq[h] / (double)c), h};
    if (better(b, mine)) mine = b;
  }
  best[threadIdx.x] = mine;
  __syncthreads();
  for (int step = kThreads / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step && better(best[threadIdx.x + step], best[threadIdx.x])) best[threadIdx.x] = best[threadIdx.x + step];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const Best w = best[0];
  double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  if (w.count > 0) sample_similarity(seed, (unsigned long long)w.h, n, N, source, target, T);   // the bits ransac_eval_kernel used
  for (int k = 0; k < 12; k++) out[k] = T[k];
  out[12] = (double)w.count;
  out[13] = w.count > 0 ? sumsq[w.h] : 0.0;
  out[14] = w.count > 0 ? (double)w.h : -1.0;
}

}  // namespace rgev

extern "C" {

int radegs_evalio_unpack_points(long long N, int S, const void* buffer, long long byte_offset, const int* offsets3, const int* types3, double* out,
                                void* stream) {
  if (N < 0 || S < 1 || S > RADEGS_MODELIO_MAX_RECORD || byte_offset < 0 || !offsets3 || !types3) return RADEGS_ERR_INVALID_ARG;
  rgev::PointColumns c;
  for (int k = 0; k < 3; k++) {
    const int size = rgev::type_size(types3[k]);
    if (size == 0 || offsets3[k] < 0 || offsets3[k] + size > S) return RADEGS_ERR_INVALID_ARG;
    c.offset[k] = offsets3[k];
    c.type[k] = types3[k];
  }
  if (N == 0) return 0;
  if (!buffer || !out || (reinterpret_cast<uintptr_t>(buffer) & 3)) return RADEGS_ERR_INVALID_ARG;
  const long long tiles = (N + rgev::kTile - 1) / rgev::kTile;
  if (tiles > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  const size_t lds = (size_t)rgev::kTile * S + 32;
  hipLaunchKernelGGL(rgev::unpack_points_kernel, dim3((unsigned)tiles), dim3(rgev::kThreads), lds, static_cast<hipStream_t>(stream), N, S,
                     static_cast<const uint32_t*>(buffer), byte_offset, c, out);
  return rg::launch_status();
}

int radegs_evalio_unpack_faces(long long F, int S, const void* buffer, long long byte_offset, int count_offset, int count_type, int index_offset,
                               int index_type, long long V, long long* faces, unsigned int* bad, void* stream_v) {
  if (F < 0 || V < 0 || S < 1 || S > RADEGS_MODELIO_MAX_RECORD || byte_offset < 0 || !bad) return RADEGS_ERR_INVALID_ARG;
  if (count_type < RADEGS_MODELIO_I1 || count_type > RADEGS_MODELIO_U4 || (index_type != RADEGS_MODELIO_I4 && index_type != RADEGS_MODELIO_U4))
    return RADEGS_ERR_INVALID_ARG;
  if (count_offset < 0 || count_offset + rgev::type_size(count_type) > S || index_offset < 0 || index_offset + 12 > S) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (hipMemsetAsync(bad, 0, sizeof(unsigned int), s) != hipSuccess) return RADEGS_ERR_HIP;
  if (F == 0) return 0;
  if (!buffer || !faces || (reinterpret_cast<uintptr_t>(buffer) & 3)) return RADEGS_ERR_INVALID_ARG;
  const long long tiles = (F + rgev::kTile - 1) / rgev::kTile;
  if (tiles > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  const size_t lds = (size_t)rgev::kTile * S + 32;
  hipLaunchKernelGGL(rgev::unpack_faces_kernel, dim3((unsigned)tiles), dim3(rgev::kThreads), lds, s, F, S, static_cast<const uint32_t*>(buffer), byte_offset,
                     count_offset, count_type, index_offset, index_type, V, faces, bad);
  return rg::launch_status();
}

int radegs_evalio_ransac(long long N, const double* source, const double* target, double max_dist, int ransac_n, long long K, unsigned long long seed,
                         int* counts, double* sumsq, double* out15, void* stream_v) {
  if (ransac_n < RADEGS_EVALIO_RANSAC_MIN_N || ransac_n > RADEGS_EVALIO_RANSAC_MAX_N || N < ransac_n || K < 1 || !(max_dist > 0.0) || !isfinite(max_dist))
    return RADEGS_ERR_INVALID_ARG;
  if (N > 0x7fffffffLL || K > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  if (!source || !target || !counts || !sumsq || !out15) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  hipLaunchKernelGGL(rgev::ransac_eval_kernel, dim3(rg::blocks_of((size_t)K)), dim3(rgev::kThreads), 0, s, (uint32_t)N, source, target, max_dist, ransac_n, K,
                     seed, counts, sumsq);
  hipLaunchKernelGGL(rgev::ransac_select_kernel, dim3(1), dim3(rgev::kThreads), 0, s, (uint32_t)N, source, target, ransac_n, K, seed, counts, sumsq, out15);
  return rg::launch_status();
}

}  // extern "C"
