// standalone sanitizer driver of ABI 15: lfsd_group_reduce with exact-size heap buffers, fp32 and fp64, the shapes of tests/group_cases.py
#include "lfsd_capi.cpp"   // the product C ABI translation unit, compiled with -DLFSD_EMU
#include <vector>
#include <cstdio>
#include <cmath>
int main() {
  const int shapes[5][3] = {{1, 1, 1}, {2, 3, 7}, {3, 2, 16}, {67, 4, 12}, {1025, 4, 7}};      // (G, D, p)
  int bad = 0;
  for (int dtype = 0; dtype < 2; ++dtype) {
    const size_t es = dtype ? 8 : 4;
    int rc = 0, wrong = 0;
    for (const auto& sh : shapes) {
      const int G = sh[0], D = sh[1], p = sh[2];
      const size_t B = (size_t)G * D, pp = (size_t)p * p;
      auto buf = [&](size_t cnt) { return std::vector<char>(cnt * es); };
      auto set = [&](std::vector<char>& v, size_t i, double val) { if (dtype) ((double*)v.data())[i] = val; else ((float*)v.data())[i] = (float)val; };
      auto get = [&](const std::vector<char>& v, size_t i) { return dtype ? ((const double*)v.data())[i] : (double)((const float*)v.data())[i]; };
      auto loss = buf(B), grad = buf(B * p), Hm = buf(B * pp), lg = buf(G), gg = buf((size_t)G * p), Hg = buf((size_t)G * pp);
      std::vector<int> ok(B), n_ok(G);
      for (size_t b = 0; b < B; ++b) {
        ok[b] = (b % 3 != 1) && (int)(b / D) != G / 2;          // group G / 2 wholly masked
        set(loss, b, ok[b] ? 1.0 : NAN);
        for (int j = 0; j < p; ++j) set(grad, b * p + j, ok[b] ? 0.5 + j : INFINITY);
        for (size_t j = 0; j < pp; ++j) set(Hm, b * pp + j, ok[b] ? 2.0 : NAN);
      }
      for (int masked = 1; masked >= 0; --masked)      // the masked pass first: NaN / inf in the rows left out
        for (int with_H = 0; with_H < (G > 1000 ? 1 : 2); ++with_H) {      // (the 1025-group shape without H: the emulator's run time)
          if (!masked) for (size_t b = 0; b < B; ++b) if (!ok[b]) { set(loss, b, 1.0); for (int j = 0; j < p; ++j) set(grad, b * p + j, 0.5 + j); for (size_t j = 0; j < pp; ++j) set(Hm, b * pp + j, 2.0); }
          rc |= lfsd_group_reduce(dtype, G, D, p, loss.data(), grad.data(), with_H ? Hm.data() : nullptr, masked ? ok.data() : nullptr,
                                  lg.data(), gg.data(), with_H ? Hg.data() : nullptr, n_ok.data(), nullptr);
          for (int g = 0; g < G; ++g) {
            int cnt = 0;
            for (int d = 0; d < D; ++d) cnt += masked ? ok[(size_t)g * D + d] : 1;
            if (n_ok[g] != cnt || get(lg, g) != (double)cnt || get(gg, (size_t)g * p + p - 1) != cnt * (0.5 + p - 1)) ++wrong;
            if (with_H && get(Hg, (size_t)g * pp + pp - 1) != 2.0 * cnt) ++wrong;
          }
        }
    }
    printf("dtype %d groups rc %d wrong %d\n", dtype, rc, wrong);
    if (rc != 0 || wrong != 0) bad = 1;
  }
  return bad;
}
