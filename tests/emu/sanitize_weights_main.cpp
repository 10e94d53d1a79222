// standalone sanitizer driver of ABI 16: the three weighted entry points with exact-size heap buffers, fp32 and fp64, both interpolation
// levels -- NULL weights, all-zero and mixed weights, poisoned padding (NaN / 1e30 in the taus and targets of zero-weight slots); every
// output sits between guard words that are checked after each call (tests/test_weights_emu.py)
#include "lfsd_capi.cpp"   // the product C ABI translation unit, compiled with -DLFSD_EMU
#include <vector>
#include <cstdio>
#include <cstring>
#include <cmath>
int main() {
  lfsd_model_info mi; lfsd_get_model_info(&mi);
  const int N = 4, B = 5, K = 5, n = mi.n_state, m = mi.n_control, p = mi.n_auxvar, nc = mi.n_const, ni = 1, GUARD = 8;
  int bad = 0;
  for (int dtype = 0; dtype < 2; ++dtype) {
    const size_t es = dtype ? 8 : 4;
    auto buf = [&](size_t cnt) { return std::vector<char>(cnt * es); };
    auto set = [&](std::vector<char>& v, size_t i, double val) { if (dtype) ((double*)v.data())[i] = val; else ((float*)v.data())[i] = (float)val; };
    auto get = [&](const std::vector<char>& v, size_t i) { return dtype ? ((const double*)v.data())[i] : (double)((const float*)v.data())[i]; };
    // an output of `cnt` elements inside GUARD elements of 777 on either side
    auto guarded = [&](size_t cnt) { auto v = buf(cnt + 2 * GUARD); for (size_t i = 0; i < cnt + 2 * GUARD; ++i) set(v, i, 777.0); return v; };
    auto intact = [&](const std::vector<char>& v) { const size_t cnt = v.size() / es; for (int i = 0; i < GUARD; ++i) if (get(v, i) != 777.0 || get(v, cnt - 1 - i) != 777.0) return false; return true; };
    auto x0 = buf(B * n), hz = buf(B), th = buf(B * p), cs = buf(nc ? nc : 1), X = buf(B * (N + 1) * n), U = buf(B * (N + 1) * m),
         L = buf(B * (N + 1) * n), cost = buf(B), Z = buf((size_t)B * (N + 1) * (n + p) * n), cX = buf(B * (N + 1) * n), cU = buf(B * (N + 1) * m),
         cL = buf(B * (N + 1) * n), taus = buf(B * K), wps = buf(B * K * ni), wts = buf(B * K), aX = buf((size_t)B * (N + 1) * p * n),
         aU = buf((size_t)B * (N + 1) * p * m);
    for (int b = 0; b < B; ++b) { set(hz, b, 1.0 + 0.05 * b); for (int i = 0; i < p; ++i) set(th, b * p + i, 1.0 + 0.1 * i + 0.05 * b); }
    for (int i = 0; i < nc; ++i) set(cs, i, lfsd_const_default(i));
    std::vector<int> it(B), st(B), iface = {0}, stats(4 * B);
    size_t wsb = lfsd_coc_workspace_bytes(dtype, B, N, 3, LFSD_MAP_LOCKSTEP, 0);
    std::vector<char> ws(wsb);
    int rc = lfsd_coc_solve(dtype, B, N, 4, x0.data(), hz.data(), th.data(), nc ? cs.data() : nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0,
                            X.data(), U.data(), L.data(), cost.data(), it.data(), st.data(), 40, dtype ? 1e-9 : 1e-6, 3, LFSD_MAP_LOCKSTEP, ws.data(), wsb, nullptr);
    rc |= lfsd_grid_curvature(dtype, B, N, n, X.data(), cX.data(), nullptr) | lfsd_grid_curvature(dtype, B, N, m, U.data(), cU.data(), nullptr) |
          lfsd_grid_curvature(dtype, B, N, n, L.data(), cL.data(), nullptr);
    st[1] = LFSD_ST_FAILED;                      // row 1 is skipped: NaN outputs, no neighbour touched
    int wrong = 0;
    // pass 0: NULL weights; 1: all zero, every tau and target poisoned; 2: mixed -- row b keeps the slots (b + j) % K != 0, 1 with weights
    // 0.25 .. 3.5, the two others are poisoned
    for (int level = 1; level <= 2; ++level)
      for (int pass = 0; pass < 3; ++pass) {
        for (int b = 0; b < B; ++b)
          for (int w = 0; w < K; ++w) {
            const bool gone = pass == 1 || (pass == 2 && (b + w) % K < 2);
            set(wts, b * K + w, gone ? 0.0 : 0.25 + 0.75 * w + 0.05 * b);
            set(taus, b * K + w, gone ? ((w & 1) ? NAN : 1e30) : (w == 0 ? 0.0 : (w == K - 1 ? get(hz, b) : 0.23 * w * get(hz, b))));
            set(wps, b * K + w, gone ? ((w & 1) ? -1e30 : NAN) : 0.5 + 0.3 * w);
          }
        auto loss = guarded(B), grad = guarded((size_t)B * p), Hm = guarded((size_t)B * p * p);
        const void* wp = pass ? wts.data() : nullptr;
        rc |= (level == 1 ? lfsd_aux_riccati(dtype, B, N, hz.data(), th.data(), nc ? cs.data() : nullptr, 0, X.data(), U.data(), L.data(), Z.data(), 4, 0.0,
                                             stats.data(), st.data(), 1 << LFSD_ST_FAILED, nullptr)
                          : lfsd_aux_riccati_cubic(dtype, B, N, hz.data(), th.data(), nc ? cs.data() : nullptr, 0, X.data(), U.data(), L.data(), cX.data(),
                                                   cU.data(), cL.data(), Z.data(), 4, 0.0, stats.data(), st.data(), 1 << LFSD_ST_FAILED, nullptr));
        rc |= (level == 1 ? lfsd_aux_forward_weighted(dtype, B, N, hz.data(), th.data(), nc ? cs.data() : nullptr, 0, X.data(), U.data(), L.data(), Z.data(),
                                                      K, ni, iface.data(), taus.data(), wps.data(), wp, loss.data() + GUARD * es, grad.data() + GUARD * es,
                                                      aX.data(), aU.data(), 4, 0.0, stats.data(), st.data(), 1 << LFSD_ST_FAILED, nullptr)
                          : lfsd_aux_forward_cubic_weighted(dtype, B, N, hz.data(), th.data(), nc ? cs.data() : nullptr, 0, X.data(), U.data(), L.data(),
                                                            cX.data(), cU.data(), cL.data(), Z.data(), K, ni, iface.data(), taus.data(), wps.data(), wp,
                                                            loss.data() + GUARD * es, grad.data() + GUARD * es, aX.data(), aU.data(), 4, 0.0,
                                                            stats.data(), st.data(), 1 << LFSD_ST_FAILED, nullptr));
        rc |= lfsd_normal_matrix_weighted(dtype, B, N, n, p, K, ni, iface.data(), hz.data(), taus.data(), wp, aX.data(), Hm.data() + GUARD * es, nullptr);
        if (!intact(loss) || !intact(grad) || !intact(Hm)) ++wrong;
        for (int b = 0; b < B; ++b) {
          const double l = get(loss, GUARD + b), g0 = get(grad, GUARD + (size_t)b * p), h0 = get(Hm, GUARD + (size_t)b * p * p);
          // (the skipped row: NaN loss / gradient / sensitivities, so a NaN H -- unless no waypoint of it exists: nothing is read, H = 0)
          if (b == 1) { if (!std::isnan(l) || !std::isnan(g0) || (pass == 1 ? h0 != 0.0 : !std::isnan(h0))) ++wrong; continue; }
          if (pass == 1 ? (l != 0.0 || g0 != 0.0 || h0 != 0.0) : !(std::isfinite(l) && l > 0.0 && std::isfinite(g0) && std::isfinite(h0) && h0 >= 0.0)) ++wrong;
          for (int q1 = 0; q1 < p; ++q1)
            for (int q2 = 0; q2 < q1; ++q2)
              if (get(Hm, GUARD + ((size_t)b * p + q1) * p + q2) != get(Hm, GUARD + ((size_t)b * p + q2) * p + q1)) ++wrong;
        }
      }
    printf("dtype %d weights rc %d wrong %d\n", dtype, rc, wrong);
    if (rc != 0 || wrong != 0) bad = 1;
  }
  return bad;
}
