// rg_conv_chain.h -- the ONE accumulation chain of the image-evaluation 3x3 convolutions (radegs_imageeval.hip), in words
// the host compiles too (radegs_conv_chain_check.cpp builds the test-only restatement from it).
//
// An output element y[n][oy][ox][co] of a stride-1, zero-padded 3x3 convolution over Cin channels is
//     acc = bias[co];   for k = 0 .. 9 Cin - 1:   acc = fmaf(x_k, w_k, acc);   y = max(acc, 0)
// with one rounding per step and no second accumulator.  Term k is CHUNK-MAJOR: the input channels go in chunks of kChunk (16; the whole
// of Cin where Cin < 16, i.e. the first layer's 3), inside a chunk the nine taps go row by row (ky, then kx), and inside a tap the
// chunk's channels ascend:
//     k = (chunk * 9 + ky * 3 + kx) * ck + (ci - chunk * ck),   ck = min(Cin, kChunk)
//     x_k = x[n][oy + ky - 1][ox + kx - 1][ci], or 0 outside the image (the step is still taken: fmaf(0, w, acc));   w_k = w[co][ci][ky][kx]
// The device follows it because the f32-input MFMA is a k-ordered fmaf chain and the kernel feeds it k in this order.
#pragma once

#if defined(__HIPCC__)
#define RG_CHAIN_HD __host__ __device__
#else
#define RG_CHAIN_HD
#endif

namespace rgconv {

constexpr int kChunk = 16;

struct Term {
  int ci, ky, kx;
};

RG_CHAIN_HD inline int chunk_channels(int Cin) { return Cin < kChunk ? Cin : kChunk; }

RG_CHAIN_HD inline Term term(int k, int Cin) {
  const int ck = chunk_channels(Cin);
  const int chunk = k / (9 * ck), r = k - chunk * 9 * ck, tap = r / ck;
  return Term{chunk * ck + (r - tap * ck), tap / 3, tap - (tap / 3) * 3};
}

}  // namespace rgconv
