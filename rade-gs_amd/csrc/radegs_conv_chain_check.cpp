// radegs_conv_chain_check.cpp -- test-only: the host restatement of the image-evaluation convolution, one fmaf chain per output element in
// the K order of rg_conv_chain.h.  g++ builds it into libradegs_conv_chain_check.so (build.py); never linked into the product.
#include <cmath>
#include <cstddef>
#include <vector>

#include "rg_conv_chain.h"

extern "C" int radegs_conv_chain_host(int N, int H, int W, int Cin, int Cout, const float* x /* [N,H,W,Cin] */, const float* w /* [Cout,Cin,3,3] */,
                                      const float* bias /* [Cout] */, int relu, float* y /* [N,H,W,Cout] */) {
  if (N < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || !x || !w || !bias || !y) return -1;
  const int K = 9 * Cin;
  std::vector<rgconv::Term> terms(K);   // the order is the header's; only the divisions are hoisted
  for (int k = 0; k < K; k++) terms[k] = rgconv::term(k, Cin);
  for (int n = 0; n < N; n++)
    for (int oy = 0; oy < H; oy++)
      for (int ox = 0; ox < W; ox++) {
        const size_t pix = ((size_t)n * H + oy) * W + ox;
        for (int co = 0; co < Cout; co++) {
          float acc = bias[co];
          for (int k = 0; k < K; k++) {
            const rgconv::Term t = terms[k];
            const int iy = oy + t.ky - 1, ix = ox + t.kx - 1;
            const float xv = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[(((size_t)n * H + iy) * W + ix) * Cin + t.ci] : 0.0f;
            acc = std::fmaf(xv, w[(((size_t)co * Cin + t.ci) * 3 + t.ky) * 3 + t.kx], acc);
          }
          y[pix * Cout + co] = (relu && !(acc > 0.0f)) ? 0.0f : acc;
        }
      }
  return 0;
}
