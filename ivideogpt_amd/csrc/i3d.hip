// Kinetics-400 Inception-I3D on the device, inference only, fp32: the detector behind FVD (the reference's Evaluator loads it as a
// torchscript file and calls it with rescale = resize = return_features = True; ivideogpt/utils/video_metric.py:26-55).  The weights
// are the caller's (ivideogpt_amd/packing.py pack_i3d: batch norm folded into weight and bias in fp64, K ordered (kd, kh, kw, c)).
//
//   front end   (B, T, 3, H, W) fp32 / bf16 in [0, 1] -> per frame bilinear resize to S x S (align_corners = False, no antialias),
//               2 x - 1, channels-last fp32 [clip][d][h][w][c]
//   conv3d      implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32, fp32 accumulation): M = output voxels, N = Cout, K = (kd, kh, kw, c).
//               64 x 64 x 32 tiles, 4 waves of 32 x 32, operands staged through LDS (rows padded to 36 floats), the next tile's global
//               loads in flight while the current one is on the matrix cores.  Any Cin / Cout: 16-byte loads when Cin and the channel
//               strides are multiples of 4, per-element loads otherwise.  TensorFlow SAME padding: the front pad is an argument, the
//               back pad is the bounds check.  Bias + optional ReLU fused; input and output carry a channel stride (and the output a
//               channel offset), so a branch of a Mixed block writes straight into its slice of the concatenated tensor.  K is never
//               split: every output element is ONE k-ordered fma chain whatever tile or chunk it lands in -- same inputs, same bits.
//   pool3d      SAME max-pool (the padded zeros take part in the maximum), any kernel / stride, channels-last
//   head        average pool over (2, S/32, S/32) stride 1, logits (1 x 1 x 1 convolution with bias), mean over the remaining time steps
//
// The architecture is ONE table (kArch below; a Mixed block expands to b0, b1a, b1b, b2a, b2b, b3a (pool), b3b); channel counts come
// from the weight shapes, so a state dict with every width divided by 4 or 8 is a valid small detector.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ivg.h"
#include "ops.h"

namespace ivg {

void set_create_error(const std::string& s);   // api.cpp: the text behind ivg_last_error(NULL)

// --------------------------------------------------------------------------------------------------------------------- conv3d
constexpr int C3_BM = 64, C3_BN = 64, C3_BK = 32, C3_LD = 36;   // LDS rows of 32 floats padded to 36: the 16 rows of a fragment read
                                                                // start on 16 different 16-byte slots of the 256-byte bank row

struct Conv3dDev {
  const float* X; const float* W; const float* bias; float* Y;
  int D, H, Wd, Cin, ldx, Do, Ho, Wo, KD, KH, KW, sd, sh, sw, pd, ph, pw, M, N, K, ldy, coff, relu;
};

template <bool VEC>
__global__ __launch_bounds__(256) void conv3d_kernel(const Conv3dDev p) {
  __shared__ __attribute__((aligned(16))) float sA[C3_BM * C3_LD];
  __shared__ __attribute__((aligned(16))) float sB[C3_BN * C3_LD];
  const int tid = threadIdx.x, chunk = tid & 7, row0 = tid >> 3;
  const int tiles_n = (p.N + C3_BN - 1) / C3_BN;
  const int tile_n = blockIdx.x % tiles_n, tile_m = blockIdx.x / tiles_n;
  const bool single = p.KD * p.KH * p.KW == 1;

  // the two voxel rows this thread gathers, fixed for the whole K loop
  long a_base[2];
  int a_d[2], a_h[2], a_w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = tile_m * C3_BM + row0 + 32 * i;
    if (m < p.M) {
      int t = m;
      const int ow = t % p.Wo; t /= p.Wo;
      const int oh = t % p.Ho; t /= p.Ho;
      const int od = t % p.Do;
      const int n = t / p.Do;
      a_base[i] = (long)n * p.D * p.H * p.Wd;
      a_d[i] = od * p.sd - p.pd; a_h[i] = oh * p.sh - p.ph; a_w[i] = ow * p.sw - p.pw;
    } else {
      a_base[i] = 0; a_d[i] = -(1 << 24); a_h[i] = 0; a_w[i] = 0;
    }
  }

  auto load_tile = [&](int kt, f32x4* ra, f32x4* rb) {
    const int k = kt * C3_BK + chunk * 4;
    if constexpr (VEC) {   // Cin % 4 == 0: the four k of a chunk share a tap
      const bool kv = k < p.K;
      int c = k, kd = 0, kh = 0, kw = 0;
      if (!single) {
        int tap = k / p.Cin;
        c = k - tap * p.Cin;
        kw = tap % p.KW; tap /= p.KW;
        kh = tap % p.KH; kd = tap / p.KH;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int id = a_d[i] + kd, ih = a_h[i] + kh, iw = a_w[i] + kw;
        const bool ok = kv & (id >= 0) & (id < p.D) & (ih >= 0) & (ih < p.H) & (iw >= 0) & (iw < p.Wd);
        ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) ra[i] = *(const f32x4*)(p.X + (a_base[i] + ((long)id * p.H + ih) * p.Wd + iw) * p.ldx + c);
        const int n = tile_n * C3_BN + row0 + 32 * i;
        rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kv & (n < p.N)) rb[i] = *(const f32x4*)(p.W + (long)n * p.K + k);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = k + j;
        const bool kv = kk < p.K;
        int c = kk, kd = 0, kh = 0, kw = 0;
        if (!single) {
          int tap = kk / p.Cin;
          c = kk - tap * p.Cin;
          kw = tap % p.KW; tap /= p.KW;
          kh = tap % p.KH; kd = tap / p.KH;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int id = a_d[i] + kd, ih = a_h[i] + kh, iw = a_w[i] + kw;
          const bool ok = kv & (id >= 0) & (id < p.D) & (ih >= 0) & (ih < p.H) & (iw >= 0) & (iw < p.Wd);
          float x = 0.f, w = 0.f;
          if (ok) x = p.X[(a_base[i] + ((long)id * p.H + ih) * p.Wd + iw) * p.ldx + c];
          const int n = tile_n * C3_BN + row0 + 32 * i;
          if (kv & (n < p.N)) w = p.W[(long)n * p.K + kk];
          ra[i][j] = x; rb[i][j] = w;
        }
      }
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave & 1, wn = wave >> 1;
  const int lr = lane & 15, lg = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + C3_BK - 1) / C3_BK;
  f32x4 ra[2], rb[2];
  load_tile(0, ra, rb);
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(f32x4*)(sA + (row0 + 32 * i) * C3_LD + chunk * 4) = ra[i];
      *(f32x4*)(sB + (row0 + 32 * i) * C3_LD + chunk * 4) = rb[i];
    }
    __syncthreads();
    if (kt + 1 < nk) load_tile(kt + 1, ra, rb);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int c = (kk * 4 + lg) * 4;
      f32x4 xa[2], wb[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) xa[b] = *(const f32x4*)(sA + (wm * 32 + b * 16 + lr) * C3_LD + c);
#pragma unroll
      for (int a = 0; a < 2; ++a) wb[a] = *(const f32x4*)(sB + (wn * 32 + a * 16 + lr) * C3_LD + c);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[a][s], xa[b][s], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }

  // the weights are the MFMA's first operand: a lane holds 4 consecutive output channels (lg * 4 + r) of voxel lr
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int m = tile_m * C3_BM + wm * 32 + b * 16 + lr;
    if (m >= p.M) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int n0 = tile_n * C3_BN + wn * 32 + a * 16 + lg * 4;
      if (n0 >= p.N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc[a][b][r] + ((n0 + r < p.N) ? p.bias[n0 + r] : 0.f);
        if (p.relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
      }
      float* o = p.Y + (long)m * p.ldy + p.coff + n0;
      if (n0 + 3 < p.N && (((uintptr_t)o) & 15) == 0) {
        *(f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n0 + r < p.N) o[r] = v[r];
      }
    }
  }
}

int launch_conv3d(const Conv3dArgs& a, hipStream_t st) {
  if (!a.X || !a.W || !a.bias || !a.Y) return (int)hipErrorInvalidValue;
  if (a.n <= 0 || a.D <= 0 || a.H <= 0 || a.Wd <= 0 || a.Cin <= 0 || a.Cout <= 0 || a.Do <= 0 || a.Ho <= 0 || a.Wo <= 0) return (int)hipErrorInvalidValue;
  if (a.ldx < a.Cin || a.coff < 0 || a.ldy < a.coff + a.Cout) return (int)hipErrorInvalidValue;
  for (int i = 0; i < 3; ++i)
    if (a.k[i] < 1 || a.k[i] > 7 || a.s[i] < 1 || a.s[i] > 2 || a.p[i] < 0 || a.p[i] >= a.k[i]) return (int)hipErrorInvalidValue;
  const long M = (long)a.n * a.Do * a.Ho * a.Wo, K = (long)a.k[0] * a.k[1] * a.k[2] * a.Cin;
  const long tiles = (long)cdiv(M, C3_BM) * cdiv(a.Cout, C3_BN);
  if (M > 0x7fffffffL || K > 0x7fffffffL || tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  Conv3dDev d{a.X, a.W, a.bias, a.Y, a.D, a.H, a.Wd, a.Cin, a.ldx, a.Do, a.Ho, a.Wo, a.k[0], a.k[1], a.k[2], a.s[0], a.s[1], a.s[2],
              a.p[0], a.p[1], a.p[2], (int)M, a.Cout, (int)K, a.ldy, a.coff, a.relu};
  const bool vec = a.Cin % 4 == 0 && a.ldx % 4 == 0 && (((uintptr_t)a.X | (uintptr_t)a.W) & 15) == 0;
  if (vec) hipLaunchKernelGGL(conv3d_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, d);
  else hipLaunchKernelGGL(conv3d_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, d);
  return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------------------------------- pool3d
struct Pool3dDev {
  const float* X; float* Y;
  int D, H, Wd, C, ldx, Do, Ho, Wo, kd, kh, kw, sd, sh, sw, pd, ph, pw, ldy, coff;
  long total;
};

__global__ __launch_bounds__(256) void pool3d_kernel(const Pool3dDev p) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < p.total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % p.C);
    long t = idx / p.C;
    const long m = t;
    const int ow = (int)(t % p.Wo); t /= p.Wo;
    const int oh = (int)(t % p.Ho); t /= p.Ho;
    const int od = (int)(t % p.Do);
    const long n = t / p.Do;
    float best = -INFINITY;
    for (int a = 0; a < p.kd; ++a)
      for (int b = 0; b < p.kh; ++b)
        for (int e = 0; e < p.kw; ++e) {
          const int id = od * p.sd - p.pd + a, ih = oh * p.sh - p.ph + b, iw = ow * p.sw - p.pw + e;
          const bool ok = (id >= 0) & (id < p.D) & (ih >= 0) & (ih < p.H) & (iw >= 0) & (iw < p.Wd);
          const float v = ok ? p.X[(((n * p.D + id) * p.H + ih) * p.Wd + iw) * p.ldx + c] : 0.f;   // a tap outside the tensor is SAME padding
          best = fmaxf(best, v);
        }
    p.Y[m * p.ldy + p.coff + c] = best;
  }
}

int launch_pool3d(const Pool3dArgs& a, hipStream_t st) {
  if (!a.X || !a.Y || a.n <= 0 || a.D <= 0 || a.H <= 0 || a.Wd <= 0 || a.C <= 0 || a.Do <= 0 || a.Ho <= 0 || a.Wo <= 0) return (int)hipErrorInvalidValue;
  if (a.ldx < a.C || a.coff < 0 || a.ldy < a.coff + a.C) return (int)hipErrorInvalidValue;
  for (int i = 0; i < 3; ++i)
    if (a.k[i] < 1 || a.k[i] > 7 || a.s[i] < 1 || a.s[i] > 2 || a.p[i] < 0 || a.p[i] >= a.k[i]) return (int)hipErrorInvalidValue;
  Pool3dDev d{a.X, a.Y, a.D, a.H, a.Wd, a.C, a.ldx, a.Do, a.Ho, a.Wo, a.k[0], a.k[1], a.k[2], a.s[0], a.s[1], a.s[2], a.p[0], a.p[1], a.p[2],
              a.ldy, a.coff, (long)a.n * a.Do * a.Ho * a.Wo * a.C};
  const int blocks = (int)std::min<long>(65536, (d.total + 255) / 256);
  hipLaunchKernelGGL(pool3d_kernel, dim3(blocks), dim3(256), 0, st, d);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------------------------- head
// avg[(n, t, c)] = mean of X[n][t .. t + 1][all pixels][c]: one fp32 chain in (dt, pixel) order
__global__ __launch_bounds__(256) void i3d_avg_kernel(const float* __restrict__ X, float* __restrict__ avg, long total, int D, int P, int C) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C);
    const long t = idx / C;
    const int d = (int)(t % (D - 1));
    const long n = t / (D - 1);
    const float* x = X + ((n * D + d) * P) * C + c;
    float s = 0.f;
    for (int i = 0; i < 2 * P; ++i) s += x[(long)i * C];
    avg[idx] = s / (float)(2 * P);
  }
}

// one wave per (clip, output): per time step the dot product (lane-strided fma chains, butterfly sum) plus bias, then the mean over time
__global__ __launch_bounds__(256) void i3d_logits_kernel(const float* __restrict__ avg, const float* __restrict__ W, const float* __restrict__ bias,
                                                         float* __restrict__ out, int Tn, int C, int Nout) {
  const int n = blockIdx.x, j = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Nout) return;
  const float* w = W + (long)j * C;
  float tot = 0.f;
  for (int t = 0; t < Tn; ++t) {
    const float* a = avg + ((long)n * Tn + t) * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(a[c], w[c], s);
    tot += wave_sum(s) + bias[j];
  }
  if (lane == 0) out[(long)n * Nout + j] = tot / (float)Tn;
}

size_t i3d_head_ws_bytes(int n, int D, int C) { return (n <= 0 || D < 2 || C <= 0) ? 0 : (size_t)n * (D - 1) * C * sizeof(float); }

int launch_i3d_head(const float* X, const float* W, const float* bias, float* out, int n, int D, int P, int C, int Nout, float* ws, hipStream_t st) {
  if (!X || !W || !bias || !out || !ws || n <= 0 || D < 2 || P <= 0 || C <= 0 || Nout <= 0) return (int)hipErrorInvalidValue;
  const long total = (long)n * (D - 1) * C;
  hipLaunchKernelGGL(i3d_avg_kernel, dim3((unsigned)std::min<long>(65536, (total + 255) / 256)), dim3(256), 0, st, X, ws, total, D, P, C);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(i3d_logits_kernel, dim3((unsigned)n, (unsigned)cdiv(Nout, 4)), dim3(256), 0, st, (const float*)ws, W, bias, out, D - 1, C, Nout);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ front end
// PyTorch's bilinear, align_corners = False: source index ((2 o + 1) H - S) / (2 S) clamped at 0, computed in integers so the
// interpolation weight is the exact rational rounded once.
template <typename TI>
__global__ __launch_bounds__(256) void i3d_ingest_kernel(const TI* __restrict__ src, float* __restrict__ Y, long total, int H, int W, int S) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int ox = (int)(idx % S);
    long t = idx / S;
    const int oy = (int)(t % S);
    const long f = t / S;
    long ny = (long)(2 * oy + 1) * H - S, nx = (long)(2 * ox + 1) * W - S;
    ny = ny < 0 ? 0 : ny; nx = nx < 0 ? 0 : nx;
    const int y0 = (int)(ny / (2 * S)), x0 = (int)(nx / (2 * S));
    const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const float ly = (float)(ny - (long)y0 * 2 * S) / (float)(2 * S), lx = (float)(nx - (long)x0 * 2 * S) / (float)(2 * S);
    const float hy = 1.0f - ly, hx = 1.0f - lx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const TI* p = src + (f * 3 + c) * H * W;
      const float top = hx * to_f32(p[(long)y0 * W + x0]) + lx * to_f32(p[(long)y0 * W + x1]);
      const float bot = hx * to_f32(p[(long)y1 * W + x0]) + lx * to_f32(p[(long)y1 * W + x1]);
      Y[idx * 3 + c] = 2.0f * (hy * top + ly * bot) - 1.0f;
    }
  }
}

int launch_i3d_ingest(const void* video, DType dt, float* Y, long frames, int H, int W, int S, hipStream_t st) {
  if (!video || !Y || frames <= 0 || H <= 0 || W <= 0 || S <= 0) return (int)hipErrorInvalidValue;
  const long total = frames * S * S;
  const unsigned blocks = (unsigned)std::min<long>(65536, (total + 255) / 256);
  if (dt == BF16) hipLaunchKernelGGL(i3d_ingest_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)video, Y, total, H, W, S);
  else hipLaunchKernelGGL(i3d_ingest_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)video, Y, total, H, W, S);
  return (int)hipGetLastError();
}

// strided channel slice -> contiguous rows (the tap of a unit that wrote into a concatenated tensor)
__global__ __launch_bounds__(256) void i3d_slice_copy_kernel(const float* __restrict__ X, float* __restrict__ Y, long total, int C, int ld, int coff) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) Y[idx] = X[(idx / C) * ld + coff + idx % C];
}

// --------------------------------------------------------------------------------------------------------------- architecture
enum { U_CONV = 0, U_POOL = 1, U_MIXED = 2 };
struct ArchRow { const char* name; int kind; int k[3]; int s[3]; };
static const ArchRow kArch[] = {
    {"Conv3d_1a_7x7", U_CONV, {7, 7, 7}, {2, 2, 2}},
    {"MaxPool3d_2a_3x3", U_POOL, {1, 3, 3}, {1, 2, 2}},
    {"Conv3d_2b_1x1", U_CONV, {1, 1, 1}, {1, 1, 1}},
    {"Conv3d_2c_3x3", U_CONV, {3, 3, 3}, {1, 1, 1}},
    {"MaxPool3d_3a_3x3", U_POOL, {1, 3, 3}, {1, 2, 2}},
    {"Mixed_3b", U_MIXED, {}, {}},
    {"Mixed_3c", U_MIXED, {}, {}},
    {"MaxPool3d_4a_3x3", U_POOL, {3, 3, 3}, {2, 2, 2}},
    {"Mixed_4b", U_MIXED, {}, {}},
    {"Mixed_4c", U_MIXED, {}, {}},
    {"Mixed_4d", U_MIXED, {}, {}},
    {"Mixed_4e", U_MIXED, {}, {}},
    {"Mixed_4f", U_MIXED, {}, {}},
    {"MaxPool3d_5a_2x2", U_POOL, {2, 2, 2}, {2, 2, 2}},
    {"Mixed_5b", U_MIXED, {}, {}},
    {"Mixed_5c", U_MIXED, {}, {}},
};
// the units of a Mixed block, in unit order; the block's output is cat(b0, b1b, b2b, b3b) on channels
static const ArchRow kMixed[7] = {
    {"b0", U_CONV, {1, 1, 1}, {1, 1, 1}},  {"b1a", U_CONV, {1, 1, 1}, {1, 1, 1}}, {"b1b", U_CONV, {3, 3, 3}, {1, 1, 1}},
    {"b2a", U_CONV, {1, 1, 1}, {1, 1, 1}}, {"b2b", U_CONV, {3, 3, 3}, {1, 1, 1}}, {"b3a", U_POOL, {3, 3, 3}, {1, 1, 1}},
    {"b3b", U_CONV, {1, 1, 1}, {1, 1, 1}},
};

struct Unit {
  std::string name;
  int kind;
  int k[3], s[3];
  int cin = 0, cout = 0;
  const float* w = nullptr;
  const float* b = nullptr;
};

struct I3dNet {
  int device = 0, resize = 0;
  std::vector<Unit> units;
  const float* lw = nullptr;
  const float* lb = nullptr;
  int feat_c = 0, n_out = 0;
};

static int same_out(int n, int s) { return (n + s - 1) / s; }
static int same_front(int n, int k, int s) { return (n % s == 0 ? std::max(k - s, 0) : std::max(k - n % s, 0)) / 2; }

I3dNet* i3d_create(const ivg_tensor* weights, int n_weights, int device, int resize, int* status_out) {
  int status = IVG_OK;
  auto find = [&](const std::string& name, int64_t* rows, int64_t* cols) -> const float* {
    for (int i = 0; i < n_weights; ++i) {
      if (!weights[i].name || name != weights[i].name) continue;
      const ivg_tensor& t = weights[i];
      const bool ok = t.dtype == IVG_F32 && t.data && !((uintptr_t)t.data & 15) && t.ndim >= 1 && t.ndim <= 2 && t.shape[0] > 0 &&
                      (t.ndim == 1 || t.shape[1] > 0) && t.shape[0] < (1 << 24) && (t.ndim == 1 || t.shape[1] < (1 << 28));
      if (!ok) {
        if (status == IVG_OK) { status = IVG_ERR_INVALID; set_create_error("I3D weight tensor '" + name + "': expected a 16-byte aligned float32 matrix or vector"); }
        return nullptr;
      }
      *rows = t.shape[0]; *cols = t.ndim == 2 ? t.shape[1] : 1;
      return (const float*)t.data;
    }
    if (status == IVG_OK) { status = IVG_ERR_MISSING; set_create_error("missing I3D weight tensor '" + name + "'"); }
    return nullptr;
  };
  auto bad = [&](const std::string& name, const std::string& why) {
    if (status == IVG_OK) { status = IVG_ERR_INVALID; set_create_error("I3D weight tensor '" + name + "': " + why); }
  };
  I3dNet net;
  net.device = device; net.resize = resize;
  auto add = [&](const std::string& name, const ArchRow& r, int cin) -> int {   // -> channels after the unit
    Unit u;
    u.name = name; u.kind = r.kind;
    for (int i = 0; i < 3; ++i) { u.k[i] = r.k[i]; u.s[i] = r.s[i]; }
    u.cin = u.cout = cin;
    if (r.kind == U_CONV) {
      int64_t rows = 0, cols = 0, brows = 0, bcols = 0;
      u.w = find(name + ".weight", &rows, &cols);
      u.b = find(name + ".bias", &brows, &bcols);
      const int64_t taps = (int64_t)r.k[0] * r.k[1] * r.k[2];
      if (u.w && cols != taps * cin) bad(name + ".weight", "expected " + std::to_string(taps * cin) + " columns (" + std::to_string(taps) + " taps x " +
                                                             std::to_string(cin) + " input channels), got " + std::to_string(cols));
      if (u.w && u.b && (brows != rows || bcols != 1)) bad(name + ".bias", "expected " + std::to_string(rows) + " elements");
      u.cout = (int)rows;
    }
    net.units.push_back(u);
    return u.cout;
  };
  int c = 3;
  for (const ArchRow& r : kArch) {
    if (status != IVG_OK) break;
    if (r.kind != U_MIXED) { c = add(r.name, r, c); continue; }
    const std::string p = std::string(r.name) + ".";
    const int o0 = add(p + "b0", kMixed[0], c);
    const int o2 = add(p + "b1b", kMixed[2], add(p + "b1a", kMixed[1], c));
    const int o4 = add(p + "b2b", kMixed[4], add(p + "b2a", kMixed[3], c));
    const int o5 = add(p + "b3b", kMixed[6], add(p + "b3a", kMixed[5], c));
    c = o0 + o2 + o4 + o5;
  }
  if (status == IVG_OK) {
    int64_t rows = 0, cols = 0, brows = 0, bcols = 0;
    net.lw = find("logits.weight", &rows, &cols);
    net.lb = find("logits.bias", &brows, &bcols);
    if (net.lw && cols != c) bad("logits.weight", "expected " + std::to_string(c) + " columns, got " + std::to_string(cols));
    if (net.lw && net.lb && (brows != rows || bcols != 1)) bad("logits.bias", "expected " + std::to_string(rows) + " elements");
    net.feat_c = c; net.n_out = (int)rows;
  }
  *status_out = status;
  return status == IVG_OK ? new I3dNet(net) : nullptr;
}

void i3d_destroy(I3dNet* p) { delete p; }
int i3d_features_dim(const I3dNet* p) { return p->n_out; }
int i3d_units(const I3dNet* p) { return (int)p->units.size(); }

// -------------------------------------------------------------------------------------------------------------------- forward
// Four scratch buffers per chunk: 0 / 1 ping-pong the trunk, 2 holds a branch's 1 x 1 x 1 output (and the head's averages), 3 the
// pooled input of branch 3.  A dry run sizes them (floats per clip) with the code that launches.
struct TRef { int buf, D, H, W, C, ld, coff; };

struct Run {
  const I3dNet* net;
  int n = 0;                 // clips of the chunk
  bool dry = true;
  float* base[4] = {};
  long need[4] = {};         // floats per clip
  hipStream_t st = nullptr;
  int tap_unit = -2;         // -1: the front end's output
  float* tap_out = nullptr;  // the chunk's first clip in the caller's tensor
  TRef tapped{};
  int tap_src[4] = {-2, -2, -2, -2};
  void note(const TRef& t) { need[t.buf] = std::max(need[t.buf], (long)t.D * t.H * t.W * t.ld); }
};

// 0: went on; 1: the tap was taken, stop; otherwise a HIP error
static int take_tap(Run& r, int u, const TRef& t, const int* src) {
  if (u != r.tap_unit) return 0;
  r.tapped = t;
  for (int i = 0; i < 4; ++i) r.tap_src[i] = src[i];
  if (!r.dry) {
    const long total = (long)r.n * t.D * t.H * t.W * t.C;
    hipLaunchKernelGGL(i3d_slice_copy_kernel, dim3((unsigned)std::min<long>(65536, (total + 255) / 256)), dim3(256), 0, r.st,
                       (const float*)r.base[t.buf], r.tap_out, total, t.C, t.ld, t.coff);
    if (int rc = (int)hipGetLastError()) return rc;
  }
  return 1;
}

static int exec_unit(Run& r, int ui, const TRef& in, TRef& out, const int* src) {
  const Unit& u = r.net->units[ui];
  int p[3];
  const int dims[3] = {in.D, in.H, in.W};
  for (int i = 0; i < 3; ++i) p[i] = same_front(dims[i], u.k[i], u.s[i]);
  out.D = same_out(in.D, u.s[0]); out.H = same_out(in.H, u.s[1]); out.W = same_out(in.W, u.s[2]);
  if (in.C != u.cin || out.C != u.cout) return (int)hipErrorInvalidValue;
  r.note(out);
  if (!r.dry) {
    int rc;
    if (u.kind == U_CONV) {
      Conv3dArgs a{r.base[in.buf] + in.coff, u.w, u.b, r.base[out.buf], r.n, in.D, in.H, in.W, in.C, in.ld, out.D, out.H, out.W,
                   {u.k[0], u.k[1], u.k[2]}, {u.s[0], u.s[1], u.s[2]}, {p[0], p[1], p[2]}, u.cout, out.ld, out.coff, 1};
      rc = launch_conv3d(a, r.st);
    } else {
      Pool3dArgs a{r.base[in.buf] + in.coff, r.base[out.buf], r.n, in.D, in.H, in.W, in.C, in.ld, out.D, out.H, out.W,
                   {u.k[0], u.k[1], u.k[2]}, {u.s[0], u.s[1], u.s[2]}, {p[0], p[1], p[2]}, out.ld, out.coff};
      rc = launch_pool3d(a, r.st);
    }
    if (rc) return rc;
  }
  return take_tap(r, ui, out, src);
}

// the trunk over the chunk whose resized input sits in buffer 0; *last: the tensor in front of the head
static int forward(Run& r, int T, int S, TRef* last) {
  const I3dNet& net = *r.net;
  TRef cur{0, T, S, S, 3, 3, 0};
  r.note(cur);
  int src[4] = {-2, -2, -2, -2};   // the units whose outputs, concatenated, are `cur`
  if (int rc = take_tap(r, -1, cur, src)) return rc;
  src[0] = -1;
  int u = 0;
#define I3D_TRY(x) do { if (int rc_ = (x)) return rc_; } while (0)
  for (const ArchRow& row : kArch) {
    if (row.kind != U_MIXED) {
      TRef out{cur.buf ^ 1, 0, 0, 0, net.units[u].cout, net.units[u].cout, 0};
      I3D_TRY(exec_unit(r, u, cur, out, src));
      cur = out;
      src[0] = u; src[1] = src[2] = src[3] = -2;
      u += 1;
      continue;
    }
    const Unit* m = &net.units[u];
    const int o0 = m[0].cout, o2 = m[2].cout, o4 = m[4].cout, o5 = m[6].cout, ctot = o0 + o2 + o4 + o5;
    auto slice = [&](int coff, int c) { return TRef{cur.buf ^ 1, 0, 0, 0, c, ctot, coff}; };
    auto temp = [&](int buf, int c) { return TRef{buf, 0, 0, 0, c, c, 0}; };
    const int one[4][4] = {{u + 1, -2, -2, -2}, {u + 3, -2, -2, -2}, {u + 5, -2, -2, -2}};
    TRef b0 = slice(0, o0), b1a = temp(2, m[1].cout), b1b = slice(o0, o2), b2a = temp(2, m[3].cout), b2b = slice(o0 + o2, o4),
         b3a = temp(3, cur.C), b3b = slice(o0 + o2 + o4, o5);
    I3D_TRY(exec_unit(r, u + 0, cur, b0, src));
    I3D_TRY(exec_unit(r, u + 1, cur, b1a, src));
    I3D_TRY(exec_unit(r, u + 2, b1a, b1b, one[0]));
    I3D_TRY(exec_unit(r, u + 3, cur, b2a, src));
    I3D_TRY(exec_unit(r, u + 4, b2a, b2b, one[1]));
    I3D_TRY(exec_unit(r, u + 5, cur, b3a, src));
    I3D_TRY(exec_unit(r, u + 6, b3a, b3b, one[2]));
    cur = TRef{cur.buf ^ 1, b0.D, b0.H, b0.W, ctot, ctot, 0};
    src[0] = u; src[1] = u + 2; src[2] = u + 4; src[3] = u + 6;
    u += 7;
  }
#undef I3D_TRY
  if (cur.D >= 2) r.need[2] = std::max(r.need[2], (long)(cur.D - 1) * cur.C);
  *last = cur;
  return 0;
}

static int side_of(const I3dNet* p, int H, int W) { return p->resize > 0 ? p->resize : (H == W ? H : -1); }

// 0 when (T, H, W) is a clip the detector takes: a side that is a multiple of 32, two time steps at least in front of the average pool
int i3d_check_shape(const I3dNet* p, int T, int H, int W) {
  const int S = side_of(p, H, W);
  if (T <= 0 || H <= 0 || W <= 0 || S <= 0 || S % 32 != 0 || S > 4096 || T > 4096) return -1;
  return same_out(same_out(same_out(T, 2), 2), 2) >= 2 ? 0 : -1;
}

static size_t clip_bytes(const Run& r) {
  size_t b = 0;
  for (int i = 0; i < 4; ++i) b += (((size_t)r.need[i] * sizeof(float)) + 255) & ~(size_t)255;
  return b;
}

static void carve(Run& r, void* ws, int n) {
  char* p = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  for (int i = 0; i < 4; ++i) { r.base[i] = (float*)p; p += ((((size_t)r.need[i] * sizeof(float)) + 255) & ~(size_t)255) * n; }
}

size_t i3d_ws_bytes(const I3dNet* p, int max_clips, int T, int H, int W) {
  if (max_clips <= 0 || i3d_check_shape(p, T, H, W)) return 0;
  Run r; r.net = p;
  TRef last;
  if (forward(r, T, side_of(p, H, W), &last)) return 0;
  return clip_bytes(r) * max_clips + 256;
}

// -4: the workspace does not hold one clip
int i3d_features(const I3dNet* p, const void* video, DType dt, int B, int T, int H, int W, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
  const int S = side_of(p, H, W);
  Run r; r.net = p;
  TRef last;
  if (int rc = forward(r, T, S, &last)) return rc;
  const size_t per = clip_bytes(r);
  const long cap = ws_bytes < 256 ? 0 : (long)((ws_bytes - 256) / per);
  if (cap < 1) return -4;
  const int N = (int)std::min<long>(cap, B);
  carve(r, ws, N);
  r.dry = false; r.st = st;
  const size_t esz = dt == BF16 ? 2 : 4;
  for (int i0 = 0; i0 < B; i0 += N) {
    r.n = std::min(N, B - i0);
    if (int rc = launch_i3d_ingest((const char*)video + (size_t)i0 * T * 3 * H * W * esz, dt, r.base[0], (long)r.n * T, H, W, S, st)) return rc;
    if (int rc = forward(r, T, S, &last)) return rc;
    if (int rc = launch_i3d_head(r.base[last.buf], p->lw, p->lb, out + (long)i0 * p->n_out, r.n, last.D, last.H * last.W, last.C, p->n_out, r.base[2], st))
      return rc;
  }
  return 0;
}

// dims[8] = D, H, W, C of the tap and the (up to four) units whose concatenated outputs the unit reads (-1: the front end, -2: none).
// out == nullptr: the dims alone.  -1: no such unit; -4: the workspace does not hold one clip.
int i3d_tap(const I3dNet* p, const void* video, DType dt, int B, int T, int H, int W, int unit, float* out, int64_t* dims, void* ws, size_t ws_bytes,
            hipStream_t st) {
  const int S = side_of(p, H, W);
  if (unit < -1 || unit >= (int)p->units.size()) return -1;
  Run r; r.net = p; r.tap_unit = unit;
  TRef last;
  if (forward(r, T, S, &last) != 1) return -1;
  const TRef t = r.tapped;
  if (dims) {
    dims[0] = t.D; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C;
    for (int i = 0; i < 4; ++i) dims[4 + i] = r.tap_src[i];
  }
  if (!out) return 0;
  Run full; full.net = p;           // buffers sized as for a whole forward: the chunking of a tap equals that of ivg_i3d_features
  if (int rc = forward(full, T, S, &last)) return rc;
  const size_t per = clip_bytes(full);
  const long cap = ws_bytes < 256 ? 0 : (long)((ws_bytes - 256) / per);
  if (cap < 1) return -4;
  const int N = (int)std::min<long>(cap, B);
  for (int i = 0; i < 4; ++i) r.need[i] = full.need[i];
  carve(r, ws, N);
  r.dry = false; r.st = st;
  const size_t esz = dt == BF16 ? 2 : 4;
  const long per_clip = (long)t.D * t.H * t.W * t.C;
  for (int i0 = 0; i0 < B; i0 += N) {
    r.n = std::min(N, B - i0);
    r.tap_out = out + (long)i0 * per_clip;
    if (int rc = launch_i3d_ingest((const char*)video + (size_t)i0 * T * 3 * H * W * esz, dt, r.base[0], (long)r.n * T, H, W, S, st)) return rc;
    const int rc = forward(r, T, S, &last);
    if (rc != 1) return rc ? rc : (int)hipErrorUnknown;
  }
  return 0;
}

}  // namespace ivg
