// MaxPool2d(2, 2) of the vgg_cnn front end (reference: models/asr/transformer.py:46,52; the view / transpose of :74-76 folded into the
// second pool's layout): HBM-bound streaming kernels.  Layouts: NHWC in; out NHWC (`nhwc`) or the encoder's (B, W/2, C, H/2) (`tcf`,
// staged through LDS; `tcf_vec` with 16-byte accesses on both sides).  The *_code forms trade the pre-pool activations for one selection
// byte per pooled element.
#include "conv_common.h"

namespace {

// ================================================================================================ max pooling
// grid.y = pooled rows (b, oh), grid.x * 256 threads = (ow, 16-byte channel group) items of a row
template <typename T>
__global__ __launch_bounds__(256) void pool_fwd_nhwc_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W2 * groups) return;
  const int cg = t % groups, ow = t / groups;
  const int oh = blockIdx.y % H2;
  const int64_t b = blockIdx.y / H2;
  const T* base = x + (((b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
  Chunk<T> a, bq, c, d, o;
  a.v = *reinterpret_cast<const uint4*>(base);
  bq.v = *reinterpret_cast<const uint4*>(base + C);
  c.v = *reinterpret_cast<const uint4*>(base + (int64_t)W * C);
  d.v = *reinterpret_cast<const uint4*>(base + (int64_t)W * C + C);
#pragma unroll
  for (int j = 0; j < EPC; ++j) {
    const float m = fmaxf(fmaxf(DT<T>::from(a.e[j]), DT<T>::from(bq.e[j])), fmaxf(DT<T>::from(c.e[j]), DT<T>::from(d.e[j])));
    o.e[j] = DT<T>::to(m);
  }
  *reinterpret_cast<uint4*>(y + (((b * H2 + oh) * (int64_t)W2 + ow) * C) + cg * EPC) = o.v;
}
// block per (b, ow): pooled (H2, C) slab -> LDS -> written as (C, H2) i.e. feature index c*H2 + oh (transformer.py:74-76)
template <typename T>
__global__ __launch_bounds__(256) void pool_fwd_tcf_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C) {
  extern __shared__ float sp[];     // [H2][C+1]
  const int H2 = H / 2, W2 = W / 2;
  const int ow = blockIdx.x % W2, b = blockIdx.x / W2;
  for (int i = threadIdx.x; i < H2 * C; i += 256) {
    const int c = i % C, oh = i / C;
    const T* base = x + ((((int64_t)b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + c;
    const float m = fmaxf(fmaxf(DT<T>::ld(base), DT<T>::ld(base + C)),
                          fmaxf(DT<T>::ld(base + (int64_t)W * C), DT<T>::ld(base + (int64_t)W * C + C)));
    sp[oh * (C + 1) + c] = m;
  }
  __syncthreads();
  T* out = y + ((int64_t)b * W2 + ow) * (int64_t)C * H2;
  for (int i = threadIdx.x; i < H2 * C; i += 256) {
    const int oh = i % H2, c = i / H2;
    DT<T>::st(out + i, sp[oh * (C + 1) + c]);
  }
}
// The same with 16-byte accesses on both sides (C and H2 multiples of the chunk): a thread pools EPC channels of one window row
// from four 16-byte loads, and writes EPC consecutive features c*H2 + oh .. oh + EPC - 1 (gathered from LDS) as one 16-byte store.
template <typename T>
__global__ __launch_bounds__(256) void pool_fwd_tcf_vec_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float sp[];     // [H2][C+1]
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC;
  const int ow = blockIdx.x % W2, b = blockIdx.x / W2;
  for (int i = threadIdx.x; i < H2 * groups; i += 256) {
    const int cg = i % groups, oh = i / groups;
    const T* base = x + ((((int64_t)b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
    Chunk<T> a, bb, c, d;
    a.v = *reinterpret_cast<const uint4*>(base);
    bb.v = *reinterpret_cast<const uint4*>(base + C);
    c.v = *reinterpret_cast<const uint4*>(base + (int64_t)W * C);
    d.v = *reinterpret_cast<const uint4*>(base + (int64_t)W * C + C);
#pragma unroll
    for (int j = 0; j < EPC; ++j)
      sp[oh * (C + 1) + cg * EPC + j] = fmaxf(fmaxf(DT<T>::from(a.e[j]), DT<T>::from(bb.e[j])), fmaxf(DT<T>::from(c.e[j]), DT<T>::from(d.e[j])));
  }
  __syncthreads();
  T* out = y + ((int64_t)b * W2 + ow) * (int64_t)C * H2;
  const int hg = H2 / EPC;
  for (int i = threadIdx.x; i < C * hg; i += 256) {
    const int c = i / hg, oh0 = (i % hg) * EPC;
    Chunk<T> o;
#pragma unroll
    for (int j = 0; j < EPC; ++j) o.e[j] = DT<T>::to(sp[(oh0 + j) * (C + 1) + c]);
    *reinterpret_cast<uint4*>(out + c * H2 + oh0) = o.v;
  }
}
// dx for one 2x2 window: gradient goes to the FIRST maximum in scan order (PyTorch max_pool2d), times ReLU'(x)
template <typename T>
__device__ __forceinline__ void pool_bwd_window(const T* __restrict__ x, T* __restrict__ dx, int64_t base, int C, int W, float gy) {
  const float v0 = DT<T>::ld(x + base), v1 = DT<T>::ld(x + base + C);
  const float v2 = DT<T>::ld(x + base + (int64_t)W * C), v3 = DT<T>::ld(x + base + (int64_t)W * C + C);
  int arg = 0; float m = v0;
  if (v1 > m) { m = v1; arg = 1; }
  if (v2 > m) { m = v2; arg = 2; }
  if (v3 > m) { m = v3; arg = 3; }
  const float gr = m > 0.f ? gy : 0.f;
  DT<T>::st(dx + base, arg == 0 ? gr : 0.f);
  DT<T>::st(dx + base + C, arg == 1 ? gr : 0.f);
  DT<T>::st(dx + base + (int64_t)W * C, arg == 2 ? gr : 0.f);
  DT<T>::st(dx + base + (int64_t)W * C + C, arg == 3 ? gr : 0.f);
}
// NHWC backward, one thread = EPC channels (16 bytes) of one 2x2 window: 5 vector loads, 4 vector stores.
// grid.y = pooled rows (b, oh), grid.x * 256 threads = (ow, channel group) items of a row.
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_nhwc_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                                            int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W2 * groups) return;
  const int cg = t % groups, ow = t / groups;
  const int oh = blockIdx.y % H2;
  const int64_t b = blockIdx.y / H2;
  const int64_t rowp = (int64_t)W * C;
  const int64_t base = (((b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
  Chunk<T> v0, v1, v2, v3, g, o0, o1, o2, o3;
  v0.v = *reinterpret_cast<const uint4*>(x + base);
  v1.v = *reinterpret_cast<const uint4*>(x + base + C);
  v2.v = *reinterpret_cast<const uint4*>(x + base + rowp);
  v3.v = *reinterpret_cast<const uint4*>(x + base + rowp + C);
  g.v = *reinterpret_cast<const uint4*>(dy + (((b * H2 + oh) * (int64_t)W2 + ow) * C) + cg * EPC);
#pragma unroll
  for (int j = 0; j < EPC; ++j) {
    const float a0 = DT<T>::from(v0.e[j]), a1 = DT<T>::from(v1.e[j]), a2 = DT<T>::from(v2.e[j]), a3 = DT<T>::from(v3.e[j]);
    int arg = 0; float m = a0;                      // the FIRST maximum in scan order takes the gradient (PyTorch max_pool2d)
    if (a1 > m) { m = a1; arg = 1; }
    if (a2 > m) { m = a2; arg = 2; }
    if (a3 > m) { m = a3; arg = 3; }
    const T gr = m > 0.f ? g.e[j] : DT<T>::to(0.f); // times ReLU'(x)
    const T zero = DT<T>::to(0.f);
    o0.e[j] = arg == 0 ? gr : zero;
    o1.e[j] = arg == 1 ? gr : zero;
    o2.e[j] = arg == 2 ? gr : zero;
    o3.e[j] = arg == 3 ? gr : zero;
  }
  *reinterpret_cast<uint4*>(dx + base) = o0.v;
  *reinterpret_cast<uint4*>(dx + base + C) = o1.v;
  *reinterpret_cast<uint4*>(dx + base + rowp) = o2.v;
  *reinterpret_cast<uint4*>(dx + base + rowp + C) = o3.v;
}
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_tcf_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                                           int B, int H, int W, int C) {
  extern __shared__ float sp[];     // [H2][C+1]
  const int H2 = H / 2, W2 = W / 2;
  const int ow = blockIdx.x % W2, b = blockIdx.x / W2;
  const T* in = dy + ((int64_t)b * W2 + ow) * (int64_t)C * H2;
  for (int i = threadIdx.x; i < H2 * C; i += 256) {
    const int oh = i % H2, c = i / H2;
    sp[oh * (C + 1) + c] = DT<T>::ld(in + i);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H2 * C; i += 256) {
    const int c = i % C, oh = i / C;
    pool_bwd_window<T>(x, dx, ((((int64_t)b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + c, C, W, sp[oh * (C + 1) + c]);
  }
}
// The same with 16-byte accesses: dy (C, H2) comes in as chunks of EPC consecutive oh of one channel, the 2x2 windows go out as in
// pool_bwd_nhwc_kernel (EPC channels per thread: four 16-byte loads, four 16-byte stores).
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_tcf_vec_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                                               int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float sp[];     // [H2][C+1]
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC, hg = H2 / EPC;
  const int ow = blockIdx.x % W2, b = blockIdx.x / W2;
  const T* in = dy + ((int64_t)b * W2 + ow) * (int64_t)C * H2;
  for (int i = threadIdx.x; i < C * hg; i += 256) {
    const int c = i / hg, oh0 = (i % hg) * EPC;
    Chunk<T> g;
    g.v = *reinterpret_cast<const uint4*>(in + c * H2 + oh0);
#pragma unroll
    for (int j = 0; j < EPC; ++j) sp[(oh0 + j) * (C + 1) + c] = DT<T>::from(g.e[j]);
  }
  __syncthreads();
  const int64_t rowp = (int64_t)W * C;
  for (int i = threadIdx.x; i < H2 * groups; i += 256) {
    const int cg = i % groups, oh = i / groups;
    const int64_t base = ((((int64_t)b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
    Chunk<T> v0, v1, v2, v3, o0, o1, o2, o3;
    v0.v = *reinterpret_cast<const uint4*>(x + base);
    v1.v = *reinterpret_cast<const uint4*>(x + base + C);
    v2.v = *reinterpret_cast<const uint4*>(x + base + rowp);
    v3.v = *reinterpret_cast<const uint4*>(x + base + rowp + C);
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      const float a0 = DT<T>::from(v0.e[j]), a1 = DT<T>::from(v1.e[j]), a2 = DT<T>::from(v2.e[j]), a3 = DT<T>::from(v3.e[j]);
      int arg = 0; float m = a0;                      // the FIRST maximum in scan order takes the gradient (PyTorch max_pool2d)
      if (a1 > m) { m = a1; arg = 1; }
      if (a2 > m) { m = a2; arg = 2; }
      if (a3 > m) { m = a3; arg = 3; }
      const T gr = DT<T>::to(m > 0.f ? sp[oh * (C + 1) + cg * EPC + j] : 0.f);       // times ReLU'(x)
      const T zero = DT<T>::to(0.f);
      o0.e[j] = arg == 0 ? gr : zero;
      o1.e[j] = arg == 1 ? gr : zero;
      o2.e[j] = arg == 2 ? gr : zero;
      o3.e[j] = arg == 3 ? gr : zero;
    }
    *reinterpret_cast<uint4*>(dx + base) = o0.v;
    *reinterpret_cast<uint4*>(dx + base + C) = o1.v;
    *reinterpret_cast<uint4*>(dx + base + rowp) = o2.v;
    *reinterpret_cast<uint4*>(dx + base + rowp + C) = o3.v;
  }
}
// ---- pooling with a selection code.  The backward kernels above find the arg max again from the pre-pool activations: for the
// first pool of the VGG front end that is 527 MB read back per step (and the only reason conv.2's full-resolution output is
// stored at all).  The *_code forms write one byte per POOLED element next to it -- 0: the maximum is <= 0 (ReLU'(x) = 0, no
// gradient), 1 + k: gradient to window position k in scan order (the FIRST maximum, PyTorch max_pool2d) -- and the backward reads
// dy and the codes only.  Code layout = layout of the pooled tensor.
__device__ __forceinline__ uint32_t pool_code(float a0, float a1, float a2, float a3, float* mx) {
  int arg = 0; float m = a0;
  if (a1 > m) { m = a1; arg = 1; }
  if (a2 > m) { m = a2; arg = 2; }
  if (a3 > m) { m = a3; arg = 3; }
  *mx = m;
  return m > 0.f ? (uint32_t)(1 + arg) : 0u;
}
template <typename T>
__global__ __launch_bounds__(256) void pool_fwd_tcf_code_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ code,
                                                                int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float sp[];     // [H2][C+1] maxima, then [H2][C+4] code bytes
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC;
  uint8_t* sc = reinterpret_cast<uint8_t*>(sp + H2 * (C + 1));
  const int ow = blockIdx.x % W2, b = blockIdx.x / W2;
  for (int i = threadIdx.x; i < H2 * groups; i += 256) {
    const int cg = i % groups, oh = i / groups;
    const T* base = x + ((((int64_t)b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
    Chunk<T> a, bb, c, d;
    a.v = *reinterpret_cast<const uint4*>(base);
    bb.v = *reinterpret_cast<const uint4*>(base + C);
    c.v = *reinterpret_cast<const uint4*>(base + (int64_t)W * C);
    d.v = *reinterpret_cast<const uint4*>(base + (int64_t)W * C + C);
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      float m;
      const uint32_t k = pool_code(DT<T>::from(a.e[j]), DT<T>::from(bb.e[j]), DT<T>::from(c.e[j]), DT<T>::from(d.e[j]), &m);
      sp[oh * (C + 1) + cg * EPC + j] = m;
      sc[oh * (C + 4) + cg * EPC + j] = (uint8_t)k;
    }
  }
  __syncthreads();
  const int64_t o0 = ((int64_t)b * W2 + ow) * (int64_t)C * H2;
  const int hg = H2 / EPC;
  for (int i = threadIdx.x; i < C * hg; i += 256) {
    const int c = i / hg, oh0 = (i % hg) * EPC;
    Chunk<T> o;
    union { uint8_t b[EPC]; uint32_t w[EPC / 4]; } k;
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      o.e[j] = DT<T>::to(sp[(oh0 + j) * (C + 1) + c]);
      k.b[j] = sc[(oh0 + j) * (C + 4) + c];
    }
    *reinterpret_cast<uint4*>(y + o0 + c * H2 + oh0) = o.v;
#pragma unroll
    for (int w = 0; w < EPC / 4; ++w) *reinterpret_cast<uint32_t*>(code + o0 + c * H2 + oh0 + 4 * w) = k.w[w];
  }
}
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_tcf_code_kernel(const uint8_t* __restrict__ code, const T* __restrict__ dy, T* __restrict__ dx,
                                                                int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ float sp[];     // [H2][C+1] gradients, then [H2][C+4] code bytes
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC, hg = H2 / EPC;
  uint8_t* sc = reinterpret_cast<uint8_t*>(sp + H2 * (C + 1));
  const int ow = blockIdx.x % W2, b = blockIdx.x / W2;
  const int64_t o0 = ((int64_t)b * W2 + ow) * (int64_t)C * H2;
  // H2 % EPC != 0 (pooled heights 20 and 10 of 80 and 40 feature rows): a channel's H2 values are no whole 16-byte chunks, so the pixel's
  // C * H2 gradients and codes are read one element per thread, still consecutive along the row; the stores below are unchanged
  if (H2 % EPC != 0)
    for (int i = threadIdx.x; i < C * H2; i += 256) {
      const int c = i / H2, oh = i % H2;
      sp[oh * (C + 1) + c] = DT<T>::from(dy[o0 + i]);
      sc[oh * (C + 4) + c] = code[o0 + i];
    }
  else
  for (int i = threadIdx.x; i < C * hg; i += 256) {
    const int c = i / hg, oh0 = (i % hg) * EPC;
    Chunk<T> g;
    g.v = *reinterpret_cast<const uint4*>(dy + o0 + c * H2 + oh0);
    union { uint8_t b[EPC]; uint32_t w[EPC / 4]; } k;
#pragma unroll
    for (int w = 0; w < EPC / 4; ++w) k.w[w] = *reinterpret_cast<const uint32_t*>(code + o0 + c * H2 + oh0 + 4 * w);
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      sp[(oh0 + j) * (C + 1) + c] = DT<T>::from(g.e[j]);
      sc[(oh0 + j) * (C + 4) + c] = k.b[j];
    }
  }
  __syncthreads();
  const int64_t rowp = (int64_t)W * C;
  for (int i = threadIdx.x; i < H2 * groups; i += 256) {
    const int cg = i % groups, oh = i / groups;
    const int64_t base = ((((int64_t)b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
    Chunk<T> o0v, o1v, o2v, o3v;
    const T zero = DT<T>::to(0.f);
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      const T gr = DT<T>::to(sp[oh * (C + 1) + cg * EPC + j]);
      const uint32_t k = sc[oh * (C + 4) + cg * EPC + j];
      o0v.e[j] = k == 1u ? gr : zero;
      o1v.e[j] = k == 2u ? gr : zero;
      o2v.e[j] = k == 3u ? gr : zero;
      o3v.e[j] = k == 4u ? gr : zero;
    }
    *reinterpret_cast<uint4*>(dx + base) = o0v.v;
    *reinterpret_cast<uint4*>(dx + base + C) = o1v.v;
    *reinterpret_cast<uint4*>(dx + base + rowp) = o2v.v;
    *reinterpret_cast<uint4*>(dx + base + rowp + C) = o3v.v;
  }
}
// NHWC forward with codes (models without the fused conv epilogue) and backward from codes: one thread = EPC channels of a window
template <typename T>
__global__ __launch_bounds__(256) void pool_fwd_nhwc_code_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ code,
                                                                 int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W2 * groups) return;
  const int cg = t % groups, ow = t / groups;
  const int oh = blockIdx.y % H2;
  const int64_t b = blockIdx.y / H2;
  const int64_t rowp = (int64_t)W * C;
  const int64_t base = (((b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
  Chunk<T> v0, v1, v2, v3, o;
  v0.v = *reinterpret_cast<const uint4*>(x + base);
  v1.v = *reinterpret_cast<const uint4*>(x + base + C);
  v2.v = *reinterpret_cast<const uint4*>(x + base + rowp);
  v3.v = *reinterpret_cast<const uint4*>(x + base + rowp + C);
  union { uint8_t b[EPC]; uint32_t w[EPC / 4]; } k;
#pragma unroll
  for (int j = 0; j < EPC; ++j) {
    float m;
    k.b[j] = (uint8_t)pool_code(DT<T>::from(v0.e[j]), DT<T>::from(v1.e[j]), DT<T>::from(v2.e[j]), DT<T>::from(v3.e[j]), &m);
    o.e[j] = DT<T>::to(m);
  }
  const int64_t po = (((b * H2 + oh) * (int64_t)W2 + ow) * C) + cg * EPC;
  *reinterpret_cast<uint4*>(y + po) = o.v;
#pragma unroll
  for (int w = 0; w < EPC / 4; ++w) *reinterpret_cast<uint32_t*>(code + po + 4 * w) = k.w[w];
}
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_nhwc_code_kernel(const uint8_t* __restrict__ code, const T* __restrict__ dy, T* __restrict__ dx,
                                                                 int B, int H, int W, int C) {
  constexpr int EPC = DT<T>::EPC;
  const int H2 = H / 2, W2 = W / 2, groups = C / EPC;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W2 * groups) return;
  const int cg = t % groups, ow = t / groups;
  const int oh = blockIdx.y % H2;
  const int64_t b = blockIdx.y / H2;
  const int64_t rowp = (int64_t)W * C;
  const int64_t base = (((b * H + 2 * oh) * W + 2 * ow) * (int64_t)C) + cg * EPC;
  const int64_t po = (((b * H2 + oh) * (int64_t)W2 + ow) * C) + cg * EPC;
  Chunk<T> g, o0, o1, o2, o3;
  g.v = *reinterpret_cast<const uint4*>(dy + po);
  union { uint8_t b[EPC]; uint32_t w[EPC / 4]; } k;
#pragma unroll
  for (int w = 0; w < EPC / 4; ++w) k.w[w] = *reinterpret_cast<const uint32_t*>(code + po + 4 * w);
  const T zero = DT<T>::to(0.f);
#pragma unroll
  for (int j = 0; j < EPC; ++j) {
    o0.e[j] = k.b[j] == 1 ? g.e[j] : zero;
    o1.e[j] = k.b[j] == 2 ? g.e[j] : zero;
    o2.e[j] = k.b[j] == 3 ? g.e[j] : zero;
    o3.e[j] = k.b[j] == 4 ? g.e[j] : zero;
  }
  *reinterpret_cast<uint4*>(dx + base) = o0.v;
  *reinterpret_cast<uint4*>(dx + base + C) = o1.v;
  *reinterpret_cast<uint4*>(dx + base + rowp) = o2.v;
  *reinterpret_cast<uint4*>(dx + base + rowp + C) = o3.v;
}
// rows/cols that floor-mode pooling drops (odd H or W) get zero gradient: touch only those pixels
template <typename T>
__global__ __launch_bounds__(256) void pool_bwd_edges_kernel(T* __restrict__ dx, int B, int H, int W, int C) {
  const int er = H & 1, ec = W & 1;
  const int64_t per_img = (int64_t)er * W + (int64_t)ec * (H - er);       // dropped pixels per image
  const int64_t total = (int64_t)B * per_img * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t e = (i / C) % per_img;
    const int64_t b = i / (C * per_img);
    int yh, xw;
    if (e < (int64_t)er * W) { yh = H - 1; xw = (int)e; }
    else { yh = (int)(e - (int64_t)er * W); xw = W - 1; }
    DT<T>::st(dx + (((b * H + yh) * W + xw) * (int64_t)C) + c, 0.f);
  }
}

// launch geometry of the two families: nhwc -- grid.y = pooled rows, grid.x * 256 threads = the (ow, 16-byte channel group) items of a row;
// tcf -- a workgroup per (b, ow) staging H2 x (C + 1) floats (+ H2 x (C + 4) selection bytes in the code forms)
dim3 pool_nhwc_grid(int B, int H2, int W2, int groups) { return dim3((unsigned)ceil_div64((int64_t)W2 * groups, 256), (unsigned)(B * H2)); }
size_t pool_tcf_lds(int H2, int C, bool code) { return (size_t)H2 * (C + 1) * sizeof(float) + (code ? (size_t)H2 * (C + 4) : 0); }

// zero gradient for the row / column that floor-mode pooling drops (odd H or W); nothing to do otherwise
int pool_bwd_edges(void* dx, int B, int H, int W, int C, int dtype, hipStream_t s) {
  if (!((H & 1) || (W & 1))) return ASR_OK;
  const int64_t total = (int64_t)B * ((int64_t)(H & 1) * W + (int64_t)(W & 1) * (H - (H & 1))) * C;
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return asr_launch<pool_bwd_edges_kernel<T>>(dim3(stream_grid(total)), dim3(256), 0, s, (T*)dx, B, H, W, C);
  });
}

}  // namespace

extern "C" int asr_maxpool_fwd(const void* x, void* y, int B, int H, int W, int C, int out_tcf, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && y && B >= 0 && H >= 2 && W >= 2 && C > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (B == 0) return ASR_OK;
  const int epc = dtype == ASR_F32 ? 4 : 8;
  const int H2 = H / 2, W2 = W / 2;
  AsrProfScope prof(ASR_OP_POOL, s);
  const size_t lds = pool_tcf_lds(H2, C, false);
  const bool vec = C % epc == 0 && H2 % epc == 0 && aligned16(x) && aligned16(y);
  if (out_tcf && lds > 150 * 1024) return ASR_EUNSUPPORTED;
  if (!out_tcf && (C % epc != 0 || !aligned16(x) || !aligned16(y))) return ASR_EUNSUPPORTED;
  if (!out_tcf && (int64_t)B * H2 > 65535) return ASR_EUNSUPPORTED;
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (!out_tcf) return asr_launch<pool_fwd_nhwc_kernel<T>>(pool_nhwc_grid(B, H2, W2, C / epc), dim3(256), 0, s, (const T*)x, (T*)y, B, H, W, C);
    if (vec) return asr_launch<pool_fwd_tcf_vec_kernel<T>>(dim3(B * W2), dim3(256), lds, s, (const T*)x, (T*)y, B, H, W, C);
    return asr_launch<pool_fwd_tcf_kernel<T>>(dim3(B * W2), dim3(256), lds, s, (const T*)x, (T*)y, B, H, W, C);
  });
}

extern "C" int asr_maxpool_bwd(const void* x, const void* dy, void* dx, int B, int H, int W, int C, int in_tcf, int dtype,
                               hipStream_t s) {
  ASR_CHECK_ARG(x && dy && dx && B >= 0 && H >= 2 && W >= 2 && C > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (B == 0) return ASR_OK;
  const int epc = dtype == ASR_F32 ? 4 : 8;
  const int H2 = H / 2, W2 = W / 2;
  AsrProfScope prof(ASR_OP_POOL, s);
  const int rc = pool_bwd_edges(dx, B, H, W, C, dtype, s);
  if (rc != ASR_OK) return rc;
  const size_t lds = pool_tcf_lds(H2, C, false);
  const bool vec = C % epc == 0 && H2 % epc == 0 && aligned16(x) && aligned16(dy) && aligned16(dx);
  if (in_tcf && lds > 150 * 1024) return ASR_EUNSUPPORTED;
  if (!in_tcf && (C % epc != 0 || !aligned16(x) || !aligned16(dy) || !aligned16(dx))) return ASR_EUNSUPPORTED;
  if (!in_tcf && (int64_t)B * H2 > 65535) return ASR_EUNSUPPORTED;
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const T *X = static_cast<const T*>(x), *DY = static_cast<const T*>(dy);
    T* DX = static_cast<T*>(dx);
    if (!in_tcf) return asr_launch<pool_bwd_nhwc_kernel<T>>(pool_nhwc_grid(B, H2, W2, C / epc), dim3(256), 0, s, X, DY, DX, B, H, W, C);
    if (vec) return asr_launch<pool_bwd_tcf_vec_kernel<T>>(dim3(B * W2), dim3(256), lds, s, X, DY, DX, B, H, W, C);
    return asr_launch<pool_bwd_tcf_kernel<T>>(dim3(B * W2), dim3(256), lds, s, X, DY, DX, B, H, W, C);
  });
}

// ---- pooling with selection codes (see pool_fwd_tcf_code_kernel): 16-byte layouts only, ASR_EUNSUPPORTED otherwise (callers then
// use asr_maxpool_fwd / asr_maxpool_bwd, which need the pre-pool activations)
extern "C" int asr_maxpool_fwd_code(const void* x, void* y, uint8_t* code, int B, int H, int W, int C, int out_tcf, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && y && code && B >= 0 && H >= 2 && W >= 2 && C > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  const int epc = dtype == ASR_F32 ? 4 : 8;
  const int H2 = H / 2, W2 = W / 2;
  if (C % epc != 0 || !aligned16(x) || !aligned16(y) || (((uintptr_t)code) & 3) != 0) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_POOL, s);
  const size_t lds = pool_tcf_lds(H2, C, true);
  if (out_tcf && (lds > 150 * 1024 || H2 % epc != 0)) return ASR_EUNSUPPORTED;
  if (!out_tcf && (int64_t)B * H2 > 65535) return ASR_EUNSUPPORTED;
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (!out_tcf) return asr_launch<pool_fwd_nhwc_code_kernel<T>>(pool_nhwc_grid(B, H2, W2, C / epc), dim3(256), 0, s, (const T*)x, (T*)y, code, B, H, W, C);
    return asr_launch<pool_fwd_tcf_code_kernel<T>>(dim3(B * W2), dim3(256), lds, s, (const T*)x, (T*)y, code, B, H, W, C);
  });
}

extern "C" int asr_maxpool_bwd_code(const uint8_t* code, const void* dy, void* dx, int B, int H, int W, int C, int in_tcf, int dtype,
                                    hipStream_t s) {
  ASR_CHECK_ARG(code && dy && dx && B >= 0 && H >= 2 && W >= 2 && C > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  const int epc = dtype == ASR_F32 ? 4 : 8;
  const int H2 = H / 2, W2 = W / 2;
  const size_t lds = pool_tcf_lds(H2, C, true);
  if (C % epc != 0 || !aligned16(dy) || !aligned16(dx) || (((uintptr_t)code) & 3) != 0) return ASR_EUNSUPPORTED;
  if (in_tcf && lds > 150 * 1024) return ASR_EUNSUPPORTED;      // any H2: whole 16-byte chunks along H2 when H2 % epc == 0, else by element
  if (!in_tcf && (int64_t)B * H2 > 65535) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_POOL, s);
  const int rc = pool_bwd_edges(dx, B, H, W, C, dtype, s);
  if (rc != ASR_OK) return rc;
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (!in_tcf) return asr_launch<pool_bwd_nhwc_code_kernel<T>>(pool_nhwc_grid(B, H2, W2, C / epc), dim3(256), 0, s, code, (const T*)dy, (T*)dx, B, H, W, C);
    return asr_launch<pool_bwd_tcf_code_kernel<T>>(dim3(B * W2), dim3(256), lds, s, code, (const T*)dy, (T*)dx, B, H, W, C);
  });
}
