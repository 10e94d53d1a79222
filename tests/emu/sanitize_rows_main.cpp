// standalone sanitizer driver of ABI 13: lfsd_optimizer_step_rows, lfsd_lookahead_rows, lfsd_trace_append with exact-size heap buffers
#include "lfsd_capi.cpp"   // the product C ABI translation unit, compiled with -DLFSD_EMU
#include <vector>
#include <cstdio>
#include <cmath>
int main() {
  const int B = 5, p = 7, capacity = 3;
  int bad = 0;
  for (int dtype = 0; dtype < 2; ++dtype) {
    const size_t es = dtype ? 8 : 4;
    auto buf = [&](size_t cnt) { return std::vector<char>(cnt * es); };
    auto set = [&](std::vector<char>& v, size_t i, double val) { if (dtype) ((double*)v.data())[i] = val; else ((float*)v.data())[i] = (float)val; };
    auto get = [&](const std::vector<char>& v, size_t i) { return dtype ? ((const double*)v.data())[i] : (double)((const float*)v.data())[i]; };
    auto th = buf(B * p), grad = buf(B * p), mm = buf(B * p), mv = buf(B * p), mvh = buf(B * p), la = buf(B * p), hyper = buf(B * 5),
         lo = buf(p), loss = buf(B), lt = buf(B * capacity), gt = buf(B * capacity), tt = buf((size_t)B * (capacity + 1) * p);
    std::vector<int> method = {0, 1, 2, 3, 4}, active = {1, 1, 0, 1, 1};
    const double hs[5] = {0.06, 0.9, 0.9, 0.999, 1e-8};
    for (int b = 0; b < B; ++b) {
      set(loss, b, 1.0 + b);
      for (int k = 0; k < 5; ++k) set(hyper, b * 5 + k, hs[k]);
      for (int j = 0; j < p; ++j) { set(th, b * p + j, 1.0 + 0.1 * j + 0.05 * b); set(grad, b * p + j, 0.3 - 0.1 * j + 0.02 * b); }
    }
    for (int j = 0; j < p; ++j) set(lo, j, j == 0 ? 1e-8 : -INFINITY);
    for (size_t i = 0; i < (size_t)B * capacity; ++i) { set(lt, i, NAN); set(gt, i, NAN); }
    for (size_t i = 0; i < (size_t)B * (capacity + 1) * p; ++i) set(tt, i, NAN);
    int rc = 0;
    for (int it = 0; it < capacity; ++it) {
      rc |= lfsd_lookahead_rows(dtype, B, p, method.data(), hyper.data(), th.data(), mm.data(), la.data(), nullptr);
      rc |= lfsd_optimizer_step_rows(dtype, B, p, it, method.data(), hyper.data(), th.data(), grad.data(), mm.data(), mv.data(), mvh.data(),
                                     lo.data(), it == 1 ? active.data() : nullptr, nullptr);
      rc |= lfsd_trace_append(dtype, B, p, it, capacity, loss.data(), grad.data(), th.data(), it == 1 ? active.data() : nullptr, lt.data(),
                              gt.data(), tt.data(), nullptr);
      // each trace alone
      rc |= lfsd_trace_append(dtype, B, p, it, capacity, loss.data(), grad.data(), th.data(), nullptr, lt.data(), nullptr, nullptr, nullptr);
      rc |= lfsd_trace_append(dtype, B, p, it, capacity, loss.data(), grad.data(), th.data(), nullptr, nullptr, gt.data(), nullptr, nullptr);
      rc |= lfsd_trace_append(dtype, B, p, it, capacity, loss.data(), grad.data(), th.data(), nullptr, nullptr, nullptr, tt.data(), nullptr);
    }
    const int over = lfsd_trace_append(dtype, B, p, capacity, capacity, loss.data(), grad.data(), th.data(), nullptr, lt.data(), gt.data(),
                                       tt.data(), nullptr);
    const bool filed = get(lt, 4 * capacity + 2) == 5.0 && get(tt, ((size_t)4 * (capacity + 1) + capacity) * p + p - 1) == get(th, 4 * p + p - 1) &&
                       std::isnan(get(tt, 0));
    printf("dtype %d rows rc %d overflow %d filed %d\n", dtype, rc, over, (int)filed);
    if (rc != 0 || over != LFSD_EINVAL || !filed) bad = 1;
  }
  return bad;
}
