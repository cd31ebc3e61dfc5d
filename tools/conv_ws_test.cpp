// Development harness for csrc/conv_ws.hip (no torch: starts in a second on a fresh GPU box).  Through the C ABI of libasr_hip.so:
//   * parity: the weight-stationary kernel (tuning WS128 = 1) against the generic implicit GEMM it replaces (WS128 = 0) AND against a
//     host loop, on exact-integer data (every partial sum is an integer below 2^24, so any summation order gives the same fp32 value
//     and the comparison is bit for bit), odd sizes, masks, both Cout, pooled form;
//   * timing at the benchmark shapes (B = 32, 80 x 400), both kernels, prefetch depth 1 / 2.
// Build:  hipcc -O2 tools/conv_ws_test.cpp -o tools/bin/conv_ws_test -Iinclude -Lend2end-asr-pytorch_amd/asr_hip -lasr_hip \
//               -Wl,-rpath,'$ORIGIN/../../end2end-asr-pytorch_amd/asr_hip'
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "asr_hip.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)
#define AK(x) do { int r_ = (x); if (r_ != 0) { fprintf(stderr, "asr error %d (%s) at %s:%d\n", r_, asr_strerror(r_), __FILE__, __LINE__); exit(3); } } while (0)

static uint16_t f2bf(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)(u >> 16); }       // exact for the small integers used here
static float bf2f(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
static uint16_t f2bf_rne(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int rint_(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

template <typename T> struct Dev {
  T* p = nullptr; size_t n = 0;
  explicit Dev(size_t n_) : n(n_) { CK(hipMalloc(&p, (n ? n : 1) * sizeof(T))); }
  ~Dev() { (void)hipFree(p); }
  void up(const std::vector<T>& h) { CK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
  std::vector<T> down() const { std::vector<T> h(n); CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return h; }
};

struct Case { int B, H, W, Cout; bool mask, relu, pooled; int Cin = 128; };
static const char* knob(const Case& c) { return c.Cin == 64 ? "WS64" : "WS128"; }      // the switch between the old and the new kernel for this shape

static int run_case(const Case& c, bool host_check) {
  const int Cin = c.Cin;
  const size_t npx = (size_t)c.B * c.H * c.W;
  std::vector<uint16_t> x(npx * Cin), wk((size_t)c.Cout * 9 * Cin), mk(npx * c.Cout);
  std::vector<float> bias(c.Cout);
  for (auto& v : x) v = f2bf((float)rint_(-3, 3));
  for (auto& v : wk) v = f2bf((float)rint_(-2, 2));
  for (auto& v : mk) v = f2bf((float)rint_(-1, 1));
  for (auto& v : bias) v = (float)rint_(-8, 8) * 0.5f;
  Dev<uint16_t> dx(x.size()), dw(wk.size()), dm(mk.size());
  Dev<float> db(bias.size());
  dx.up(x); dw.up(wk); dm.up(mk); db.up(bias);
  const size_t nout = c.pooled ? (size_t)c.B * (c.W / 2) * c.Cout * (c.H / 2) : npx * c.Cout;
  std::vector<std::vector<uint16_t>> ys(2);       // WS128 = 0 generic implicit GEMM, 1 conv_ws.hip; empty = shape unsupported
  std::vector<std::vector<uint8_t>> cds(2);
  for (int ws = 0; ws < 2; ++ws) {
    AK(asr_set_tuning(knob(c), ws));
    Dev<uint16_t> dy(nout);
    Dev<uint8_t> dc(c.pooled ? nout : 1);
    CK(hipMemset(dy.p, 0xff, nout * 2));
    if (c.pooled) {
      // the generic kernel needs H % 16 == 0, conv_ws.hip H % 8 == 0; the entry point then returns EUNSUPPORTED ... or falls through to an
      // older kernel that supports the shape: only count a result as the new kernel's when the shape is in its domain
      if ((ws == 0 && c.H % 16 != 0) || (ws == 1 && c.H % 8 != 0)) continue;
      AK(asr_conv3x3_relu_pool_tcf_code(dx.p, dw.p, db.p, dy.p, dc.p, c.B, c.H, c.W, Cin, c.Cout, ASR_BF16, nullptr));
    } else {
      AK(asr_conv3x3_igemm(dx.p, dw.p, db.p, c.mask ? dm.p : nullptr, dy.p, c.B, c.H, c.W, Cin, c.Cout, c.relu ? 1 : 0, ASR_BF16, nullptr));
    }
    CK(hipDeviceSynchronize());
    ys[ws] = dy.down();
    if (c.pooled) cds[ws] = dc.down();
  }
  AK(asr_clear_tuning(knob(c)));
  size_t bad = 0;
  if (!ys[0].empty())
    for (int k = 1; k < 2; ++k) {
      if (ys[k].empty()) continue;
      for (size_t i = 0; i < nout; ++i) bad += ys[0][i] != ys[k][i];
      if (c.pooled) for (size_t i = 0; i < nout; ++i) bad += cds[0][i] != cds[k][i];
    }
  size_t bad_host = 0;
  if (host_check) {
    std::vector<float> y(npx * c.Cout);
    for (int b = 0; b < c.B; ++b)
      for (int h = 0; h < c.H; ++h)
        for (int w = 0; w < c.W; ++w)
          for (int co = 0; co < c.Cout; ++co) {
            float s = bias[co];
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx) {
                const int yy = h + ky - 1, xx = w + kx - 1;
                if (yy < 0 || yy >= c.H || xx < 0 || xx >= c.W) continue;
                const uint16_t* xp = &x[(((size_t)b * c.H + yy) * c.W + xx) * Cin];
                const uint16_t* wp = &wk[((size_t)co * 9 + ky * 3 + kx) * Cin];
                for (int ci = 0; ci < Cin; ++ci) s += bf2f(xp[ci]) * bf2f(wp[ci]);
              }
            if (c.relu || c.pooled) s = s > 0.f ? s : 0.f;
            const size_t o = (((size_t)b * c.H + h) * c.W + w) * c.Cout + co;
            if (c.mask && !(bf2f(mk[o]) > 0.f)) s = 0.f;
            y[o] = bf2f(f2bf_rne(s));
          }
    if (!c.pooled) {
      for (int k = 1; k < 2; ++k)
        if (!ys[k].empty()) for (size_t i = 0; i < nout; ++i) bad_host += f2bf(y[i]) != ys[k][i];
    } else {
      const int H2 = c.H / 2, W2 = c.W / 2;
      for (int b = 0; b < c.B; ++b)
        for (int ow = 0; ow < W2; ++ow)
          for (int co = 0; co < c.Cout; ++co)
            for (int oh = 0; oh < H2; ++oh) {
              float m = -1.f; int arg = 0;
              for (int k = 0; k < 4; ++k) {
                const float v = y[(((size_t)b * c.H + 2 * oh + (k >> 1)) * c.W + 2 * ow + (k & 1)) * c.Cout + co];
                if (v > m) { m = v; arg = k; }
              }
              const size_t o = (((size_t)b * W2 + ow) * c.Cout + co) * H2 + oh;
              for (int k = 1; k < 2; ++k)
                if (!ys[k].empty()) bad_host += (f2bf(m) != ys[k][o]) + ((uint8_t)(m > 0.f ? 1 + arg : 0) != cds[k][o]);
            }
    }
  }
  printf("  case B=%d H=%d W=%d %d->%d mask=%d relu=%d pooled=%d : %zu mismatches vs generic kernel%s, %zu vs host%s\n", c.B, c.H, c.W, c.Cin, c.Cout,
         (int)c.mask, (int)c.relu, (int)c.pooled, bad, ys[0].empty() ? " (n/a)" : "", bad_host, host_check ? "" : " (skipped)");
  return (int)(bad + bad_host != 0);
}

static void time_case(const Case& c) {
  const int Cin = c.Cin;
  const size_t npx = (size_t)c.B * c.H * c.W;
  std::vector<uint16_t> x(npx * Cin), wk((size_t)c.Cout * 9 * Cin);
  for (auto& v : x) v = f2bf_rne((float)((int)(rnd() % 2001) - 1000) * 1e-3f);
  for (auto& v : wk) v = f2bf_rne((float)((int)(rnd() % 2001) - 1000) * 3e-5f);
  std::vector<float> bias(c.Cout, 0.01f);
  Dev<uint16_t> dx(x.size()), dw(wk.size()), dm(npx * c.Cout), dy(npx * c.Cout);
  Dev<uint8_t> dc(npx * c.Cout / 4);
  Dev<float> db(bias.size());
  dx.up(x); dw.up(wk); db.up(bias);
  CK(hipMemcpy(dm.p, dx.p, (c.Cout <= Cin ? npx * c.Cout : npx * Cin) * 2, hipMemcpyDeviceToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const double fl = 2.0 * 9 * Cin * c.Cout * (double)npx;
  for (int ws = 0; ws < 2; ++ws)
    for (int pd = 2; pd <= 2; ++pd) {        // (operand prefetch depth 1 and its WS_PD switch were removed in round 6: it lost everywhere)
      AK(asr_set_tuning(knob(c), ws));
      auto go = [&]() {
        if (c.pooled) AK(asr_conv3x3_relu_pool_tcf_code(dx.p, dw.p, db.p, dy.p, dc.p, c.B, c.H, c.W, Cin, c.Cout, ASR_BF16, nullptr));
        else AK(asr_conv3x3_igemm(dx.p, dw.p, db.p, c.mask ? dm.p : nullptr, dy.p, c.B, c.H, c.W, Cin, c.Cout, c.relu ? 1 : 0, ASR_BF16, nullptr));
      };
      for (int i = 0; i < 3; ++i) go();
      CK(hipDeviceSynchronize());
      const int iters = 20;
      CK(hipEventRecord(e0, nullptr));
      for (int i = 0; i < iters; ++i) go();
      CK(hipEventRecord(e1, nullptr));
      CK(hipEventSynchronize(e1));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double us = ms * 1e3 / iters;
      printf("  time B=%d %dx%d %d->%d mask=%d pooled=%d  %-22s %8.1f us  %7.1f TF/s (%4.1f%% of 2.5 PF)\n", c.B, c.H, c.W, c.Cin, c.Cout, (int)c.mask,
             (int)c.pooled, ws == 1 ? (pd == 2 ? "weight-stationary pd=2" : "weight-stationary pd=1") : (c.Cin == 64 ? "c64 kernel, two passes" : "generic igemm"), us, fl / us / 1e6, fl / us / 25e6);
    }
#ifdef ASR_TUNE_ABLATE        // section clocks: only a library built with ASR_HIPCC_EXTRA=-DASR_TUNE_ABLATE has the timing instantiations
  for (int ws = 1; ws < 2; ++ws) {
    if (c.Cin == 128 && ws == 1 && !(c.Cout == 128 ? (c.pooled || c.mask) : !c.mask)) continue;      // (timing instantiations of conv_ws.hip exist for these forms)
    Dev<long long> dbg(64);
    CK(hipMemset(dbg.p, 0, 64 * 8));
    AK(asr_set_tuning(knob(c), ws));
    AK(asr_set_tuning("WS_DBG", (int64_t)(uintptr_t)dbg.p));
    if (c.pooled) AK(asr_conv3x3_relu_pool_tcf_code(dx.p, dw.p, db.p, dy.p, dc.p, c.B, c.H, c.W, Cin, c.Cout, ASR_BF16, nullptr));
    else AK(asr_conv3x3_igemm(dx.p, dw.p, db.p, c.mask ? dm.p : nullptr, dy.p, c.B, c.H, c.W, Cin, c.Cout, c.relu ? 1 : 0, ASR_BF16, nullptr));
    CK(hipDeviceSynchronize());
    AK(asr_clear_tuning("WS_DBG"));
    const std::vector<long long> h = dbg.down();
    for (int w = 0; w < 4; ++w)
      printf("    %s wave %d, %lld tiles, cycles per tile: barrier %lld  staging %lld  contraction %lld  dma wait %lld  epilogue %lld\n", ws == 1 ? "ws128" : "ws16 ", w, h[w * 8 + 5],
             h[w * 8 + 0] / h[w * 8 + 5], h[w * 8 + 1] / h[w * 8 + 5], h[w * 8 + 2] / h[w * 8 + 5], h[w * 8 + 3] / h[w * 8 + 5], h[w * 8 + 4] / h[w * 8 + 5]);
  }
#endif
  AK(asr_clear_tuning(knob(c)));
}

// conv.5 forward writing its ReLU mask as bits, conv.7's data gradient reading it: both against the 16-bit-mask forms, the bits against
// the definition (include/asr_hip.h: asr_relu_bits_bytes)
static int run_bits(int B, int H, int W, bool timing) {
  const size_t npx = (size_t)B * H * W;
  std::vector<uint16_t> x(npx * 64), w5((size_t)128 * 9 * 64), g(npx * 128), w7((size_t)128 * 9 * 128);
  std::vector<float> bias(128);
  for (auto& v : x) v = f2bf((float)rint_(-3, 3));
  for (auto& v : w5) v = f2bf((float)rint_(-2, 2));
  for (auto& v : g) v = f2bf((float)rint_(-3, 3));
  for (auto& v : w7) v = f2bf((float)rint_(-2, 2));
  for (auto& v : bias) v = (float)rint_(-8, 8) * 0.5f;
  const int64_t nb = asr_relu_bits_bytes(B, H, W, 128);
  Dev<uint16_t> dx(x.size()), dw5(w5.size()), dg(g.size()), dw7(w7.size()), y0(npx * 128), y1(npx * 128), z0(npx * 128), z1(npx * 128);
  Dev<uint8_t> dbits((size_t)nb);
  Dev<float> db(128);
  dx.up(x); dw5.up(w5); dg.up(g); dw7.up(w7); db.up(bias);
  CK(hipMemset(dbits.p, 0xa5, (size_t)nb));
  AK(asr_conv3x3_igemm(dx.p, dw5.p, db.p, nullptr, y0.p, B, H, W, 64, 128, 1, ASR_BF16, nullptr));
  AK(asr_conv3x3_igemm_bits(dx.p, dw5.p, db.p, nullptr, y1.p, dbits.p, B, H, W, 64, 128, 1, ASR_BF16, nullptr));
  AK(asr_conv3x3_igemm(dg.p, dw7.p, nullptr, y0.p, z0.p, B, H, W, 128, 128, 0, ASR_BF16, nullptr));
  AK(asr_conv3x3_igemm_bits(dg.p, dw7.p, nullptr, dbits.p, z1.p, nullptr, B, H, W, 128, 128, 0, ASR_BF16, nullptr));
  CK(hipDeviceSynchronize());
  const auto hy0 = y0.down(), hy1 = y1.down(), hz0 = z0.down(), hz1 = z1.down();
  const auto hb = dbits.down();
  size_t bad_y = 0, bad_z = 0, bad_b = 0, kept = 0;
  for (size_t i = 0; i < hy0.size(); ++i) bad_y += hy0[i] != hy1[i];
  for (size_t i = 0; i < hz0.size(); ++i) bad_z += hz0[i] != hz1[i];
  const int H4 = 2 * ((H + 7) / 8), W16 = (W + 15) / 16;
  int lane_of[16][4];          // (pixel column in the tile, 8-channel chunk of the 32) -> lane: the layout of include/asr_hip.h
  for (int lane = 0; lane < 64; ++lane) {
    const int l = lane & 15, a = l >> 2, gq = lane >> 4;
    lane_of[8 * (a & 1) + 2 * (l & 3) + (((a >> 1) ^ a) & 1)][2 * (gq & 1) + (gq >> 1)] = lane;
  }
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w)
        for (int c = 0; c < 128; ++c) {
          const bool want = bf2f(hy0[(((size_t)b * H + h) * W + w) * 128 + c]) > 0.f;
          const size_t dw = ((((size_t)b * H4 + h / 4) * W16 + w / 16) * 4 + c / 32) * 64 + lane_of[w % 16][c % 32 / 8];
          const bool got = (hb[dw * 4 + h % 4] >> (c % 8)) & 1;
          bad_b += want != got;
          kept += want;
        }
  printf("  bits B=%d H=%d W=%d: conv.5 output %zu mismatches, mask bits %zu wrong (%.1f%% kept), conv.7 data gradient %zu mismatches\n", B, H, W,
         bad_y, bad_b, 100.0 * kept / (double)hy0.size(), bad_z);
  if (timing) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    // interleaved rounds (the chip's clock follows the recent load: a form timed right after another is not comparable with one
    // timed after a pause), median of 7
    static const char* names[] = {"conv.5 forward", "conv.5 forward + bits out", "conv.7 dgrad, bf16 mask", "conv.7 dgrad, bit mask"};
    std::vector<double> t[4];
    for (int round = 0; round < 7; ++round)
      for (int form = 0; form < 4; ++form) {
        auto go = [&]() {
          if (form == 0) AK(asr_conv3x3_igemm(dx.p, dw5.p, db.p, nullptr, y0.p, B, H, W, 64, 128, 1, ASR_BF16, nullptr));
          if (form == 1) AK(asr_conv3x3_igemm_bits(dx.p, dw5.p, db.p, nullptr, y1.p, dbits.p, B, H, W, 64, 128, 1, ASR_BF16, nullptr));
          if (form == 2) AK(asr_conv3x3_igemm(dg.p, dw7.p, nullptr, y0.p, z0.p, B, H, W, 128, 128, 0, ASR_BF16, nullptr));
          if (form == 3) AK(asr_conv3x3_igemm_bits(dg.p, dw7.p, nullptr, dbits.p, z1.p, nullptr, B, H, W, 128, 128, 0, ASR_BF16, nullptr));
        };
        for (int i = 0; i < 2; ++i) go();
        const int iters = 10;
        CK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) go();
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        t[form].push_back(ms * 1e3 / iters);
      }
    for (int form = 0; form < 4; ++form) {
      std::sort(t[form].begin(), t[form].end());
      printf("    time %-28s median %7.1f us  (min %7.1f, max %7.1f)\n", names[form], t[form][3], t[form][0], t[form][6]);
    }
  }
  return (bad_y || bad_z || bad_b) ? 1 : 0;
}

int main(int argc, char** argv) {
  const bool timing = argc < 2 || strcmp(argv[1], "parity") != 0;
  const bool parity = argc < 2 || strcmp(argv[1], "time") != 0;
  int fails = 0;
  if (argc >= 2 && strcmp(argv[1], "bits") == 0) {
    fails += run_bits(2, 21, 50, false);
    fails += run_bits(32, 80, 400, true);
    printf(fails ? "FAILED (%d cases)\n" : "OK\n", fails);
    return fails ? 1 : 0;
  }
  if (parity) {
    printf("== parity (exact-integer data)\n");
    const Case cases[] = {
        {1, 8, 16, 128, false, true, false},  {2, 24, 48, 128, false, true, false}, {2, 19, 37, 128, true, false, false},
        {1, 16, 32, 64, false, false, false}, {2, 21, 50, 64, true, false, false},  {3, 32, 64, 128, false, true, true},
        {2, 24, 48, 128, false, true, true},  {1, 80, 400, 128, true, false, false}, {1, 80, 400, 64, false, false, false},
        {1, 80, 400, 128, false, true, true},
    };
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) fails += run_case(cases[i], (size_t)cases[i].B * cases[i].H * cases[i].W <= 40000);
    // more workgroup-sized than the grid: persistence over many tiles, XCD walk, tail
    fails += run_case({9, 80, 400, 128, true, false, false}, false);
    fails += run_case({9, 80, 400, 128, false, true, true}, false);
    fails += run_case({9, 80, 400, 64, false, false, false}, false);
    // 64 -> 128 in one pass (conv.5 forward) against the two-pass form and the host loop
    fails += run_case({1, 8, 16, 128, false, true, false, 64}, true);
    fails += run_case({2, 21, 50, 128, false, true, false, 64}, true);
    fails += run_case({2, 24, 48, 128, false, false, false, 64}, true);
    fails += run_case({9, 80, 400, 128, false, true, false, 64}, false);
    fails += run_bits(1, 8, 16, false);
    fails += run_bits(2, 21, 50, false);
    fails += run_bits(2, 24, 48, false);
    fails += run_bits(9, 80, 400, false);
  }
  if (timing) {
    printf("== timing (B = 32, 80 x 400)\n");
    time_case({32, 80, 400, 128, false, true, true});
    time_case({32, 80, 400, 128, true, false, false});
    time_case({32, 80, 400, 128, false, true, false});
    time_case({32, 80, 400, 64, false, false, false});
    time_case({32, 80, 400, 128, false, true, false, 64});
  }
  printf(fails ? "FAILED (%d cases)\n" : "OK\n", fails);
  return fails ? 1 : 0;
}
