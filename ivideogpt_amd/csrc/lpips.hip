// LPIPS (VGG-16 variant, v0.1, spatial = False) on the device: the fourth frame metric of the reference's Evaluator.forward
// (ivideogpt/utils/video_metric.py:63-100; network: ivideogpt/vq_model/lpips.py).  fp32 throughout, as the reference forces it.
//
//   input layer   x <- ((2 x - 1) - shift) / scale fused into the 3 -> 64 convolution (planar fp32 / bf16 frames in, NHWC fp32 out,
//                 bias + ReLU): K = 27, a direct VALU kernel like conv_small.hip
//   trunk         the twelve remaining 3x3 convolutions run on the engine's fp32 MFMA instances with the IG_RELU epilogue:
//                 conv3x3.hip where it covers the shape (256-pixel tiles, width >= 16), the generic implicit GEMM below that
//   max-pool      2 x 2 / stride 2, NHWC fp32, one 16-byte vector of channels per lane
//   head          per tap ONE pass over the two feature tensors: per pixel the channel norms of both, the lin-weighted squared
//                 difference of the normalised features, summed over the pixels a workgroup owns -- neither the normalised
//                 features nor the difference are written.  Lanes -> wave (shuffles) -> workgroup (LDS) -> a partial per
//                 (image, pixel slice), reduced in a fixed order by the finish kernel: same inputs, same bits, no float atomics
//   clip reduce   per-frame values -> mean over the frames of a trajectory -> min over its samples
//
// Host side: the images go through the trunk in chunks sized by the caller's workspace, and every ground-truth frame passes the
// trunk ONCE (the reference repeats the ground truth t times): a chunk is G ground-truth frames plus, sample by sample, the
// predicted frames that pair with them.  Every per-image value is produced by the same instructions in the same order whatever
// the chunk size (kernel instances are selected by the layer's shape alone), so the result does not depend on it.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "ops.h"

namespace ivg {

static const int kTapC[5] = {64, 128, 256, 512, 512};

static std::atomic<long long> g_trunk_images{0};
long long lpips_trunk_images() { return g_trunk_images.load(std::memory_order_relaxed); }

// ---------------------------------------------------------------------------------------------------------------- input layer
// image n of the launch: sample k = k0 + n / G, ground-truth frame q = q0 + n % G of the flat (B, T) list, i.e. trajectory
// b = q / T, frame f = q % T  ->  frame (k * B + b) * T_src + t0 + f of the source clip tensor (the ground truth is launched with k0 = 0, n < G)
struct LpipsInDev {
  const void* src; const float* w; const float* bias; float* Y;
  int N, G, q0, k0, B, T, T_src, t0, H, W;
};

template <typename TI>
__global__ __launch_bounds__(256) void lpips_conv_in_kernel(const LpipsInDev p) {
  __shared__ float sw[27 * 64];   // [k = (kh, kw, ci)][co]: a lane's 8 output channels are contiguous
  __shared__ float sb[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) {
    const int co = i / 27, k = i - co * 27;   // packed source [co][kh][kw][ci]
    sw[k * 64 + co] = p.w[i];
  }
  if (threadIdx.x < 64) sb[threadIdx.x] = p.bias[threadIdx.x];
  __syncthreads();
  const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
  const long total = (long)p.N * p.H * p.W * 8;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int cg = (int)(idx & 7);
    long t = idx >> 3;
    const int ow = (int)(t % p.W); t /= p.W;
    const int oh = (int)(t % p.H);
    const int n = (int)(t / p.H);
    const int k = p.k0 + n / p.G, q = p.q0 + n % p.G;
    const int b = q / p.T, f = q - b * p.T;
    const TI* src = (const TI*)p.src + ((long)(k * p.B + b) * p.T_src + p.t0 + f) * 3 * p.H * p.W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = sb[cg * 8 + j];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = oh + kh - 1, iw = ow + kw - 1;
        const bool in = ih >= 0 && ih < p.H && iw >= 0 && iw < p.W;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          float x = 0.f;   // the zero padding is applied to the SCALED image, as the reference's conv sees it
          if (in) x = ((to_f32(src[((long)ci * p.H + ih) * p.W + iw]) * 2.0f - 1.0f) - shift[ci]) / scale[ci];
          const float* wk = sw + ((kh * 3 + kw) * 3 + ci) * 64 + cg * 8;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf(x, wk[j], acc[j]);
        }
      }
    float* o = p.Y + (((long)n * p.H + oh) * p.W + ow) * 64 + cg * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] > 0.f ? acc[j] : 0.f;
    *(f32x4*)o = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}

static int launch_lpips_conv_in(const LpipsInDev& d, DType src_dt, hipStream_t st) {
  if (d.N <= 0) return 0;
  const long total = (long)d.N * d.H * d.W * 8;
  const int blocks = (int)(total / 256 > 32768 ? 32768 : cdiv(total, 256));
  if (src_dt == BF16) hipLaunchKernelGGL(lpips_conv_in_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, d);
  else hipLaunchKernelGGL(lpips_conv_in_kernel<float>, dim3(blocks), dim3(256), 0, st, d);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------- max-pool
__global__ __launch_bounds__(256) void maxpool2_kernel(const float* __restrict__ X, float* __restrict__ Y, long total, int Ho, int Wo, int C4) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4);
    long t = idx / C4;
    const int ow = (int)(t % Wo); t /= Wo;
    const int oh = (int)(t % Ho);
    const long n = t / Ho;
    const long row = (long)2 * Wo * C4;   // 16-byte vectors per input row
    const f32x4* s = (const f32x4*)X + ((n * 2 * Ho + 2 * oh) * 2 * Wo + 2 * ow) * C4 + c;
    const f32x4 a = s[0], b = s[C4], d = s[row], e = s[row + C4];
    f32x4 m;
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = fmaxf(fmaxf(a[j], b[j]), fmaxf(d[j], e[j]));
    ((f32x4*)Y)[idx] = m;
  }
}

int launch_maxpool2(const float* X, float* Y, int N, int H, int W, int C, hipStream_t st) {
  if (N <= 0) return 0;
  if (H % 2 || W % 2 || C % 4 || H < 2 || W < 2 || ((uintptr_t)X & 15) || ((uintptr_t)Y & 15)) return (int)hipErrorInvalidValue;
  const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
  const int blocks = (int)(total / 256 > 65536 ? 65536 : cdiv(total, 256));
  hipLaunchKernelGGL(maxpool2_kernel, dim3(blocks), dim3(256), 0, st, X, Y, total, H / 2, W / 2, C / 4);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------------------------- head
// workgroup (i, s): image i of f1 against image i % n0 of f0, pixels [s * pps, min(P, (s + 1) * pps)).  LP = C / 4 lanes (64 at
// most) share a pixel, each holding NCH 16-byte vectors of its channels of both tensors; the 256 / LP pixel groups of the
// workgroup walk the slice with a fixed stride.
constexpr int LPIPS_MAX_SLICES = 16;
static int head_slices(int P) { const int s = P / 1024; return s < 1 ? 1 : (s > LPIPS_MAX_SLICES ? LPIPS_MAX_SLICES : s); }

template <int C>
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ lin,
                                                         int n0, int P, int pps, double* __restrict__ part) {
  constexpr int LP = C / 4 < 64 ? C / 4 : 64;
  constexpr int NCH = C / 4 / LP;
  constexpr int NG = 256 / LP;
  __shared__ double red[4];
  const int i = blockIdx.x, s = blockIdx.y;
  const int tid = threadIdx.x, l = tid % LP, g = tid / LP;
  const f32x4* A = (const f32x4*)f0 + (long)(i % n0) * P * (C / 4);
  const f32x4* Bv = (const f32x4*)f1 + (long)i * P * (C / 4);
  f32x4 w[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) w[j] = ((const f32x4*)lin)[l + j * LP];
  const int p1 = min(P, (s + 1) * pps);
  float acc = 0.f;
  for (int px = s * pps + g; px < p1; px += NG) {   // (the LP lanes of a pixel group leave the loop together: the shuffles stay inside it)
    f32x4 a[NCH], b[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) { a[j] = A[(long)px * (C / 4) + l + j * LP]; b[j] = Bv[(long)px * (C / 4) + l + j * LP]; }
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) { sa = fmaf(a[j][r], a[j][r], sa); sb = fmaf(b[j][r], b[j][r], sb); }
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
    const float da = sqrtf(sa) + 1e-10f, db = sqrtf(sb) + 1e-10f;   // an all-zero pixel: 0 / 1e-10 = 0
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = a[j][r] / da - b[j][r] / db;
        acc = fmaf(w[j][r], d * d, acc);
      }
  }
  const double tot = wave_sum((double)acc);
  if ((tid & 63) == 0) red[tid >> 6] = tot;
  __syncthreads();
  if (tid == 0) part[(long)i * gridDim.y + s] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[(i / n0) * group_stride + i % n0] (+)= mean over the pixels of image i
__global__ __launch_bounds__(256) void lpips_head_finish_kernel(const double* __restrict__ part, int n1, int n0, int S, int P, float* __restrict__ out,
                                                                long group_stride, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n1) return;
  double t = 0.0;
  for (int s = 0; s < S; ++s) t += part[(long)i * S + s];
  const float v = (float)(t / (double)P);
  float* o = out + (long)(i / n0) * group_stride + i % n0;
  *o = accumulate ? *o + v : v;
}

size_t lpips_head_part_bytes(int n1, int P) { return (size_t)n1 * head_slices(P) * sizeof(double); }

int launch_lpips_head(const float* f0, const float* f1, const float* lin, int n0, int n1, int P, int C, float* out, long group_stride, int accumulate,
                      double* part, hipStream_t st) {
  if (n0 <= 0 || n1 <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  if (((uintptr_t)f0 & 15) || ((uintptr_t)f1 & 15) || ((uintptr_t)lin & 15) || ((uintptr_t)part & 7)) return (int)hipErrorInvalidValue;
  const int S = head_slices(P), pps = cdiv(P, S);
  const dim3 grid((unsigned)n1, (unsigned)S);
  switch (C) {
    case 64: hipLaunchKernelGGL(lpips_head_kernel<64>, grid, dim3(256), 0, st, f0, f1, lin, n0, P, pps, part); break;
    case 128: hipLaunchKernelGGL(lpips_head_kernel<128>, grid, dim3(256), 0, st, f0, f1, lin, n0, P, pps, part); break;
    case 256: hipLaunchKernelGGL(lpips_head_kernel<256>, grid, dim3(256), 0, st, f0, f1, lin, n0, P, pps, part); break;
    case 512: hipLaunchKernelGGL(lpips_head_kernel<512>, grid, dim3(256), 0, st, f0, f1, lin, n0, P, pps, part); break;
    default: return (int)hipErrorInvalidValue;
  }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(lpips_head_finish_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, (const double*)part, n1, n0, S, P, out, group_stride, accumulate);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- clip reduce
__global__ __launch_bounds__(64) void lpips_clip_reduce_kernel(const float* __restrict__ frames, float* __restrict__ rows, int B, int t, int T) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  float best = INFINITY;
  for (int k = 0; k < t; ++k) {
    const float* f = frames + (long)(k * B + b) * T;
    double a = 0.0;
    for (int j = 0; j < T; ++j) a += f[j];
    best = fminf(best, (float)(a / T));
  }
  rows[b] = best;
}

// ---------------------------------------------------------------------------------------------------------------------- trunk
// per image, in floats: the five taps (64 + 32 + 16 + 8 + 2) HW, scratch S0 (64 HW: relu1_1) and S1 (16 HW: the widest pooled tensor)
static long tap_floats(int k, long HW) { return (long)kTapC[k] * (HW >> (2 * k)); }

struct LpipsWs {
  float* tap[5]; float* s0; float* s1; double* part;
};
static size_t lpips_img_bytes(int H, int W) {
  const long HW = (long)H * W;
  long f = 64 * HW + 16 * HW;
  for (int k = 0; k < 5; ++k) f += tap_floats(k, HW);
  return (size_t)f * sizeof(float) + LPIPS_MAX_SLICES * sizeof(double);
}
size_t lpips_ws_bytes(int max_images, int H, int W) { return max_images <= 0 ? 0 : (size_t)max_images * lpips_img_bytes(H, W) + 256; }
long lpips_ws_images(size_t ws_bytes, int H, int W) { return ws_bytes < 256 ? 0 : (long)((ws_bytes - 256) / lpips_img_bytes(H, W)); }

static LpipsWs carve(void* ws, long N, int H, int W) {
  const long HW = (long)H * W;
  char* p = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  LpipsWs r;
  r.part = (double*)p; p += (size_t)N * LPIPS_MAX_SLICES * sizeof(double);
  for (int k = 0; k < 5; ++k) { r.tap[k] = (float*)p; p += (size_t)N * tap_floats(k, HW) * sizeof(float); }
  r.s0 = (float*)p; p += (size_t)N * 64 * HW * sizeof(float);
  r.s1 = (float*)p;
  return r;
}

static int conv_relu(const float* X, float* Y, const float* w, const float* b, int n, int H, int W, int cin, int cout, hipStream_t st) {
  IgemmArgs a;
  a.X = X; a.W = w; a.Y = Y; a.bias = b;
  a.Nimg = n; a.Hin = H; a.Win = W; a.Cin = cin; a.ldx = cin; a.Hout = H; a.Wout = W;
  a.KH = 3; a.KW = 3; a.stride = 1; a.pad = 1;
  a.N = cout; a.ldw = 9 * cin;
  a.c_img = (long)H * W * cout; a.c_pix = cout; a.c_ch = 1;
  a.flags = IG_BIAS_N | IG_RELU;
  int rc = launch_conv3x3(a, F32, st);
  if (rc == -1) rc = launch_igemm(a, F32, st);
  return rc;
}

// layers 2 .. 13 over images [i0, i0 + n) of the chunk, whose relu1_1 sits in w.s0; the taps land in w.tap[k] at image i0
static int trunk_rest(const float* const* cw, const float* const* cb, const LpipsWs& w, long i0, int n, int H, int W, hipStream_t st) {
  const long HW = (long)H * W;
  float* s0 = w.s0 + i0 * 64 * HW;
  float* s1 = w.s1 + i0 * 16 * HW;
  float* tap[5];
  for (int k = 0; k < 5; ++k) tap[k] = w.tap[k] + i0 * tap_floats(k, HW);
  int rc;
#define LP_TRY(x) do { rc = (x); if (rc) return rc; } while (0)
  LP_TRY(conv_relu(s0, tap[0], cw[1], cb[1], n, H, W, 64, 64, st));
  LP_TRY(launch_maxpool2(tap[0], s1, n, H, W, 64, st));
  int h = H / 2, v = W / 2;
  LP_TRY(conv_relu(s1, s0, cw[2], cb[2], n, h, v, 64, 128, st));
  LP_TRY(conv_relu(s0, tap[1], cw[3], cb[3], n, h, v, 128, 128, st));
  LP_TRY(launch_maxpool2(tap[1], s1, n, h, v, 128, st));
  h /= 2; v /= 2;
  LP_TRY(conv_relu(s1, s0, cw[4], cb[4], n, h, v, 128, 256, st));
  LP_TRY(conv_relu(s0, s1, cw[5], cb[5], n, h, v, 256, 256, st));
  LP_TRY(conv_relu(s1, tap[2], cw[6], cb[6], n, h, v, 256, 256, st));
  LP_TRY(launch_maxpool2(tap[2], s0, n, h, v, 256, st));
  h /= 2; v /= 2;
  LP_TRY(conv_relu(s0, s1, cw[7], cb[7], n, h, v, 256, 512, st));
  LP_TRY(conv_relu(s1, s0, cw[8], cb[8], n, h, v, 512, 512, st));
  LP_TRY(conv_relu(s0, tap[3], cw[9], cb[9], n, h, v, 512, 512, st));
  LP_TRY(launch_maxpool2(tap[3], s0, n, h, v, 512, st));
  h /= 2; v /= 2;
  LP_TRY(conv_relu(s0, s1, cw[10], cb[10], n, h, v, 512, 512, st));
  LP_TRY(conv_relu(s1, s0, cw[11], cb[11], n, h, v, 512, 512, st));
  LP_TRY(conv_relu(s0, tap[4], cw[12], cb[12], n, h, v, 512, 512, st));
#undef LP_TRY
  g_trunk_images.fetch_add(n, std::memory_order_relaxed);
  return 0;
}

bool lpips_shape_ok(int H, int W) { return H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0; }

// test hook of the input layer alone: n plain images (n, 3, H, W) -> relu1_1 (n, H, W, 64)
int launch_lpips_input_layer(const void* images, DType dt, const float* w, const float* bias, float* Y, int n, int H, int W, hipStream_t st) {
  LpipsInDev d{images, w, bias, Y, n, n, 0, 0, 1, n, n, 0, H, W};
  return launch_lpips_conv_in(d, dt, st);
}

// test hook: n plain images (n, 3, H, W) through the trunk; taps_out[k] (n, H >> k, W >> k, C_k) NHWC fp32 receive copies of the taps.
// -4: the workspace does not hold one image
int launch_lpips_features(const float* const* cw, const float* const* cb, const void* images, DType dt, int n, int H, int W, float* const* taps_out,
                          void* ws, size_t ws_bytes, hipStream_t st) {
  const long N = std::min<long>(n, lpips_ws_images(ws_bytes, H, W));
  if (N < 1) return -4;
  const long HW = (long)H * W;
  const LpipsWs w = carve(ws, N, H, W);
  for (int i0 = 0; i0 < n; i0 += (int)N) {
    const int c = std::min((int)N, n - i0);
    LpipsInDev d{images, cw[0], cb[0], w.s0, c, n, i0, 0, 1, n, n, 0, H, W};
    if (int rc = launch_lpips_conv_in(d, dt, st)) return rc;
    if (int rc = trunk_rest(cw, cb, w, 0, c, H, W, st)) return rc;
    for (int k = 0; k < 5; ++k)
      if (taps_out[k] && hipMemcpyAsync(taps_out[k] + (long)i0 * tap_floats(k, HW), w.tap[k], (size_t)c * tap_floats(k, HW) * sizeof(float),
                                        hipMemcpyDeviceToDevice, st) != hipSuccess)
        return (int)hipErrorUnknown;
  }
  return 0;
}

// frames (n_samples, T): the per-frame values (always produced); -4: the workspace does not hold one image pair
int launch_lpips_rows(const float* const* cw, const float* const* cb, const float* const* lin, const void* gt, DType gt_dt, int B, int T_gt, int gt_t0,
                      const float* pred, int n_samples, int T_pr, int pr_t0, int T, int H, int W, float* frames, float* rows, void* ws, size_t ws_bytes,
                      hipStream_t st) {
  const int t = n_samples / B, Q = B * T;
  const long N = std::min<long>(lpips_ws_images(ws_bytes, H, W), (long)Q * (1 + t));
  if (N < 2) return -4;
  const int G = (int)std::max<long>(1, N / (1 + t));       // ground-truth frames per chunk
  const int KC = (int)std::min<long>(t, (N - G) / G);      // samples of them per trunk pass
  const long HW = (long)H * W;
  const LpipsWs w = carve(ws, N, H, W);
  for (int q0 = 0; q0 < Q; q0 += G) {
    const int g = std::min(G, Q - q0);
    for (int k0 = 0; k0 < t; k0 += KC) {
      const int kc = std::min(KC, t - k0), n1 = kc * g;
      // relu1_1 of the ground truth (first pass of the chunk only) into slots [0, g), of the predictions into [g, g + n1)
      if (k0 == 0) {
        LpipsInDev d{gt, cw[0], cb[0], w.s0, g, g, q0, 0, B, T, T_gt, gt_t0, H, W};
        if (int rc = launch_lpips_conv_in(d, gt_dt, st)) return rc;
      }
      LpipsInDev d{pred, cw[0], cb[0], w.s0 + (long)g * 64 * HW, n1, g, q0, k0, B, T, T_pr, pr_t0, H, W};
      if (int rc = launch_lpips_conv_in(d, F32, st)) return rc;
      if (int rc = k0 == 0 ? trunk_rest(cw, cb, w, 0, g + n1, H, W, st) : trunk_rest(cw, cb, w, g, n1, H, W, st)) return rc;
      for (int k = 0; k < 5; ++k) {
        // image j of the pass = (sample k0 + j / g, ground-truth frame q0 + j % g) -> frames[(k0 + j / g) * Q + q0 + j % g]
        if (int rc = launch_lpips_head(w.tap[k], w.tap[k] + (long)g * tap_floats(k, HW), lin[k], g, n1, (int)(HW >> (2 * k)), kTapC[k],
                                       frames + (long)k0 * Q + q0, Q, k > 0, w.part, st))
          return rc;
      }
    }
  }
  hipLaunchKernelGGL(lpips_clip_reduce_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, (const float*)frames, rows, B, t, T);
  return (int)hipGetLastError();
}

}  // namespace ivg
