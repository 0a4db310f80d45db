// Transformer-side kernels that are not GEMMs (SURVEY.md 2.4 K11, K15, K16 decode, K18, K19).
// All step-dependent scalars (cache length, index of the token being decided) live in a device-side
// StepState so the whole per-token kernel sequence has constant arguments and can be captured once
// into a hipGraph and replayed for every generated token.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "ops.h"
#include <atomic>
#include "switches.h"

namespace ivg {

// ------------------------------------------------------------------------------------------------ embedding
template <typename T>
__global__ __launch_bounds__(256) void embed_kernel(const int64_t* __restrict__ ids, long id_stride, const T* __restrict__ E,
                                                    T* __restrict__ x, long x_bstride, int L, int H, int V) {
  constexpr int VEC = Traits<T>::VEC;
  const int row = blockIdx.x;  // b * L + l
  const int b = row / L, l = row - b * L;
  long id = ids[(long)b * id_stride + l];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // memory safety only: the mirror's callers pass ids < vocab_size
  const T* src = E + id * H;
  T* dst = x + (long)b * x_bstride + (long)l * H;
  for (int c = threadIdx.x * VEC; c < H; c += 256 * VEC) *(Chunk16*)(dst + c) = *(const Chunk16*)(src + c);
}

int launch_embed(const int64_t* ids, long id_stride, const void* E, void* x, DType dt, int B, int L, int H, int V, hipStream_t st,
                 long x_bstride) {
  if (B * L <= 0) return 0;
  if (x_bstride <= 0) x_bstride = (long)L * H;
  if (dt == BF16) hipLaunchKernelGGL(embed_kernel<bf16_t>, dim3(B * L), dim3(256), 0, st, ids, id_stride, (const bf16_t*)E, (bf16_t*)x, x_bstride, L, H, V);
  else hipLaunchKernelGGL(embed_kernel<float>, dim3(B * L), dim3(256), 0, st, ids, id_stride, (const float*)E, (float*)x, x_bstride, L, H, V);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ RoPE + KV append
// thread = (row m = b*L + l, head h, pair i < hd/2).  HF rotate_half convention:
//   out[i] = x[i]*cos - x[i+hd/2]*sin ;  out[i+hd/2] = x[i+hd/2]*cos + x[i]*sin
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_kernel(T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
                                                      T* __restrict__ vt, int ldvt, const float* __restrict__ cosT,
                                                      const float* __restrict__ sinT, int B, int L, int heads, int hd, int Lmax,
                                                      const StepState* __restrict__ state, int pos0) {
  const int half = hd / 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)B * L * heads * half;
  if (idx >= total) return;
  const int i = (int)(idx % half);
  long t = idx / half;
  const int h = (int)(t % heads); t /= heads;
  const int l = (int)(t % L);
  const int b = (int)(t / L);
  const int base_pos = state ? state->pos : pos0;
  const int pos = base_pos + l;
  const int H = heads * hd;
  T* row = qkv + ((long)b * L + l) * 3 * H;
  const float c = cosT[(long)pos * half + i], s = sinT[(long)pos * half + i];
  T* q = row + h * hd;
  const float q1 = to_f32(q[i]), q2 = to_f32(q[i + half]);
  q[i] = from_f32<T>(q1 * c - q2 * s);
  q[i + half] = from_f32<T>(q2 * c + q1 * s);
  const T* k = row + H + h * hd;
  const float k1 = to_f32(k[i]), k2 = to_f32(k[i + half]);
  T* kdst = kc + (((long)b * heads + h) * Lmax + pos) * hd;
  kdst[i] = from_f32<T>(k1 * c - k2 * s);
  kdst[i + half] = from_f32<T>(k2 * c + k1 * s);
  const T* v = row + 2 * H + h * hd;
  T* vdst = vc + (((long)b * heads + h) * Lmax + pos) * hd;
  const T v1 = v[i], v2 = v[i + half];
  vdst[i] = v1;
  vdst[i + half] = v2;
  if (vt) {
    T* tb = vt + ((long)b * heads + h) * hd * ldvt;
    tb[(long)i * ldvt + l] = v1;
    tb[(long)(i + half) * ldvt + l] = v2;
  }
}

// Vectorised form for head_dim 64 prompts (pos0 known on the host): a workgroup owns ROWS consecutive positions of one
// (trajectory, head); 16-byte loads / stores throughout, and V^T leaves through an LDS transpose as whole 32-byte runs
// along the position axis (the scalar kernel above writes V^T 2 bytes at a stride of ldvt).
template <typename T>
__global__ __launch_bounds__(256) void rope_kv64_kernel(T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
                                                        T* __restrict__ vt, int ldvt, const float* __restrict__ cosT,
                                                        const float* __restrict__ sinT, int L, int heads, int Lmax, int pos0) {
  constexpr int VEC = Traits<T>::VEC, HD = 64, HALF = 32;
  constexpr int CH = HALF / VEC;        // threads per position (each owns chunk c of both halves)
  constexpr int ROWS = 256 / CH;        // positions per workgroup: 64 (bf16) / 32 (fp32)
  constexpr int PITCH = HD * (int)sizeof(T) / 4 + 1;   // dwords per staged V row: odd -> transposed reads spread over banks
  __shared__ unsigned sv[ROWS * PITCH];
  const int tid = threadIdx.x;
  const int bh = blockIdx.y, b = bh / heads, h = bh - b * heads;
  const int H = heads * HD;
  const int l0 = blockIdx.x * ROWS;
  {
    const int lr_ = tid / CH, c = tid - lr_ * CH;
    const int l = l0 + lr_;
    unsigned* dst = sv + lr_ * PITCH;
    constexpr int DW = 16 / 4;           // dwords per 16-byte chunk
    if (l < L) {
      const int pos = pos0 + l;
      T* row = qkv + ((long)b * L + l) * 3 * H + h * HD;
      float cs[VEC], sn[VEC];
#pragma unroll
      for (int j = 0; j < VEC; j += 4) {
        const f32x4 cv = *(const f32x4*)(cosT + (long)pos * HALF + c * VEC + j), sv4 = *(const f32x4*)(sinT + (long)pos * HALF + c * VEC + j);
#pragma unroll
        for (int r = 0; r < 4; ++r) { cs[j + r] = cv[r]; sn[j + r] = sv4[r]; }
      }
      auto rope = [&](T* lo_p, T* hi_p, T* lo_dst, T* hi_dst) {
        const Chunk16 lo = *(const Chunk16*)lo_p, hi = *(const Chunk16*)hi_p;
        Chunk16 olo, ohi;
        if constexpr (sizeof(T) == 2) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, lo), bb = __builtin_bit_cast(bf16x8, hi);
          bf16x8 oa, ob;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float x1 = (float)a[j], x2 = (float)bb[j];
            oa[j] = (bf16_t)(x1 * cs[j] - x2 * sn[j]);
            ob[j] = (bf16_t)(x2 * cs[j] + x1 * sn[j]);
          }
          olo = __builtin_bit_cast(Chunk16, oa); ohi = __builtin_bit_cast(Chunk16, ob);
        } else {
          const f32x4 a = __builtin_bit_cast(f32x4, lo), bb = __builtin_bit_cast(f32x4, hi);
          f32x4 oa, ob;
#pragma unroll
          for (int j = 0; j < 4; ++j) { oa[j] = a[j] * cs[j] - bb[j] * sn[j]; ob[j] = bb[j] * cs[j] + a[j] * sn[j]; }
          olo = __builtin_bit_cast(Chunk16, oa); ohi = __builtin_bit_cast(Chunk16, ob);
        }
        *(Chunk16*)lo_dst = olo; *(Chunk16*)hi_dst = ohi;
      };
      T* q = row + c * VEC;
      rope(q, q + HALF, q, q + HALF);
      T* k = row + H + c * VEC;
      T* kd = kc + ((long)bh * Lmax + pos) * HD + c * VEC;
      rope(k, k + HALF, kd, kd + HALF);
      const T* v = row + 2 * H + c * VEC;
      const Chunk16 vlo = *(const Chunk16*)v, vhi = *(const Chunk16*)(v + HALF);
      T* vd = vc + ((long)bh * Lmax + pos) * HD + c * VEC;
      *(Chunk16*)vd = vlo; *(Chunk16*)(vd + HALF) = vhi;
#pragma unroll
      for (int r = 0; r < DW; ++r) { dst[c * DW + r] = vlo[r]; dst[HALF * (int)sizeof(T) / 4 + c * DW + r] = vhi[r]; }
    } else {
#pragma unroll
      for (int r = 0; r < DW; ++r) { dst[c * DW + r] = 0u; dst[HALF * (int)sizeof(T) / 4 + c * DW + r] = 0u; }   // zero padding of V^T
    }
  }
  __syncthreads();
  if (vt) {   // thread (d, lc): ROWS / 4 consecutive positions of channel d
    constexpr int PER = ROWS / 4;
    const int d = tid >> 2, lc = tid & 3;
    const T* svT = (const T*)sv;
    T* out = vt + ((long)bh * HD + d) * ldvt + l0 + lc * PER;
    T vals[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) vals[j] = svT[(long)(lc * PER + j) * (PITCH * 4 / (int)sizeof(T)) + d];
#pragma unroll
    for (int j = 0; j < PER; j += VEC) {
      Chunk16 o;
      if constexpr (sizeof(T) == 2) { bf16x8 t8; for (int r = 0; r < 8; ++r) t8[r] = vals[j + r]; o = __builtin_bit_cast(Chunk16, t8); }
      else { f32x4 t4; for (int r = 0; r < 4; ++r) t4[r] = vals[j + r]; o = __builtin_bit_cast(Chunk16, t4); }
      *(Chunk16*)(out + j) = o;
    }
  }
}

int launch_rope_kv(void* qkv, void* kc, void* vc, void* vt, int ldvt, const float* cosT, const float* sinT, int B, int L,
                   int heads, int hd, int Lmax, const StepState* state, int pos0, DType dt, hipStream_t st) {
  const long total = (long)B * L * heads * (hd / 2);
  if (total <= 0) return 0;
  // A prompt append (no state) leaves V^T columns [L, ldvt) zero on every path: the one-pass attention and the P.V GEMM multiply
  // them by P = 0, and 0 * NaN would poison the row.  (The scalar kernel does not own those columns: a memset covers them.)
  const int rows = dt == BF16 ? 64 : 32;
  if (hd == 64 && !state && (!vt || (ldvt % rows == 0 && ldvt >= cdiv(L, rows) * rows)) && ((uintptr_t)qkv & 15) == 0) {
    dim3 g2((unsigned)(vt ? ldvt / rows : cdiv(L, rows)), (unsigned)(B * heads));   // workgroups past L only zero their V^T columns
    if (dt == BF16)
      hipLaunchKernelGGL(rope_kv64_kernel<bf16_t>, g2, dim3(256), 0, st, (bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (bf16_t*)vt, ldvt, cosT, sinT,
                         L, heads, Lmax, pos0);
    else
      hipLaunchKernelGGL(rope_kv64_kernel<float>, g2, dim3(256), 0, st, (float*)qkv, (float*)kc, (float*)vc, (float*)vt, ldvt, cosT, sinT, L,
                         heads, Lmax, pos0);
    return (int)hipGetLastError();
  }
  if (vt && !state && ldvt > L) {
    const size_t es = dt == BF16 ? 2 : 4;
    const hipError_t rc = hipMemset2DAsync((char*)vt + (size_t)L * es, (size_t)ldvt * es, 0, (size_t)(ldvt - L) * es, (size_t)B * heads * hd, st);
    if (rc != hipSuccess) return (int)rc;
  }
  dim3 g(cdiv(total, 256));
  if (dt == BF16)
    hipLaunchKernelGGL(rope_kv_kernel<bf16_t>, g, dim3(256), 0, st, (bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (bf16_t*)vt, ldvt, cosT,
                       sinT, B, L, heads, hd, Lmax, state, pos0);
  else
    hipLaunchKernelGGL(rope_kv_kernel<float>, g, dim3(256), 0, st, (float*)qkv, (float*)kc, (float*)vc, (float*)vt, ldvt, cosT, sinT,
                       B, L, heads, hd, Lmax, state, pos0);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ V^T tile of the one-pass attention kernels
// The P.V MFMA of flash_prefill_kernel / xattn_kernel enumerates the keys of a 32-key step as (4*lg + r, 16 + 4*lg + r) -- the order a
// lane's own S registers have -- so its V^T fragment is two groups of four consecutive keys, 16 apart.  Read as two 8-byte halves
// (rounds 2-4) the compiler merged them into ds_read2_b64: two accesses of 4 x 16 CONTIGUOUS lanes with banks mod 32, half the rate
// of ds_read_b128, and 2-way conflicted for 16 consecutive rows of the 144-byte pitch (the 32-38 % bank-conflict cycles of the PMC
// tables).  Now the keys of every 32-key block are PERMUTED when the tile is staged -- position lg*8 + half*4 + r holds key
// half*16 + lg*4 + r -- so a fragment is ONE conflict-free ds_read_b128.  Rows of 64 keys carry 32 bytes of pad; rows of 32 keys
// (64 bytes: the single-head 512- / 768-channel instances) use the XOR key of conv3x3's 64-byte rows instead, without pad (the
// 512-channel instance keeps two workgroups per CU).  The staging stores become two ds_write_b64 per 16-byte chunk, odd rows of the
// padded form in the other order (16 contiguous lanes = two rows then touch 32 distinct banks).  Model: tools/lds_vt_layout_check.py
// (function of the permutation + bank cycles of both access shapes).
template <int KT>
struct VtTile {
  static constexpr bool SWZ = KT == 32;
  static constexpr int PITCH = SWZ ? KT : KT + 16;   // elements
  static __device__ __forceinline__ int quad_off(int row, int quad) {   // element offset of 16-byte quad `quad` of row `row`
    if constexpr (SWZ) quad ^= (row >> 1) & 3;
    return row * PITCH + (quad << 3);
  }
  // source chunk cc of a row = its keys 8cc .. 8cc+7
  static __device__ __forceinline__ void store(bf16_t* sV, int row, int cc, Chunk16 c) {
    typedef uint32_t U2 __attribute__((ext_vector_type(2)));
    const int qa = (cc >> 2) * 4 + 2 * (cc & 1), e = ((cc >> 1) & 1) * 4;
    bf16_t* a = sV + quad_off(row, qa) + e;
    bf16_t* b = sV + quad_off(row, qa + 1) + e;
    const U2 lo = {c.x, c.y}, hi = {c.z, c.w};
    const bool odd = !SWZ && (row & 1);
    bf16_t* p0 = odd ? b : a;
    bf16_t* p1 = odd ? a : b;
    *(U2*)p0 = odd ? hi : lo;
    *(U2*)p1 = odd ? lo : hi;
  }
  // fragment of K-step pr for lane (lr, lg) of the 16-row block d: frag(sV, d * 16 + lr, pr * 4 + lg)
  static __device__ __forceinline__ bf16x8 frag(const bf16_t* sV, int row, int quad) { return *(const bf16x8*)(sV + quad_off(row, quad)); }
};

// ------------------------------------------------------------------------------------------------ prefill attention
// Causal self-attention of a prompt (positions 0 .. L-1) in one pass, bf16 / head_dim 64: replaces the score GEMM, the row
// softmax and the P.V GEMM of the prefill (and their fp32 score matrix in HBM: 910 MB per layer at config 2).
// Workgroup = 64 query rows of one (trajectory, head); wave = 16 query rows against every key tile up to the diagonal:
//   S = K Q^T      a = K rows (cache, roped), b = Q rows (roped in place by rope_kv)  -> lane: S[key = 4*lg + r][q = lr]
//   online softmax in fp32 (running max / sum per query row; a row lives in the 4 lanes lr, lr+16, lr+32, lr+48)
//   O += V^T P     a = rows of V^T (vt, [d][key]), b = P cast to bf16: the lane's own S registers ARE its P fragment when
//                  the K dimension of this MFMA enumerates the keys as (4*lg + r, 16 + 4*lg + r) -- V^T is read in the
//                  same order, so no cross-lane movement is needed          -> lane: O[d = 4*lg + r][q = lr]
// Key rows beyond the diagonal are masked by select (never by arithmetic: cache rows past L may hold anything).
__global__ __launch_bounds__(256) void flash_prefill_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc,
                                                            const bf16_t* __restrict__ vt, bf16_t* __restrict__ out, int L, int Lp,
                                                            int heads, int Lmax, float scale) {
  constexpr int HD = 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int qt = gridDim.x - 1 - blockIdx.x;   // long rows (many key tiles) are scheduled first
  const int bh = blockIdx.y, b = bh / heads, h = bh - b * heads;
  const int H = heads * HD;
  const int q = qt * 64 + wave * 16 + lr;
  const int qc = q < L ? q : L - 1;
  const bf16_t* qrow = qkv + ((long)b * L + qc) * 3 * H + h * HD;
  const bf16x8 qf0 = *(const bf16x8*)(qrow + lg * 8), qf1 = *(const bf16x8*)(qrow + 32 + lg * 8);
  const bf16_t* kb = kc + (long)bh * Lmax * HD;
  const bf16_t* vb = vt + (long)bh * HD * Lp;
  f32x4 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;
  // The four waves of the workgroup need the same 64-key tile of K and V^T: it is staged once in LDS instead of being pulled
  // from L2 by every wave, and the next tile travels from global memory into registers while the current one is consumed.
  // Row pitches per access shape (bank model of MI355X_MICROARCH.md, tools/lds_swizzle_check.py): the K rows are read back as
  // 16-byte MFMA fragments (ds_read_b128: 4 groups of 16 lanes) -- a pad of 32 bytes is conflict-free, the 16 bytes of round 2
  // cost every read a second LDS cycle (PMC: 41 % bank-conflict cycles); the V^T rows are staged key-permuted (VtTile above) and
  // read back the same way.
  using VT = VtTile<64>;
  constexpr int PITCHK = HD + 16;     // K rows
  __shared__ __attribute__((aligned(16))) bf16_t sK[64 * PITCHK];
  __shared__ __attribute__((aligned(16))) bf16_t sV[64 * VT::PITCH];
  const int srow0 = tid >> 3, scol = (tid & 7) * 8;   // this thread stages chunks (srow0, scol) and (srow0 + 32, scol)
  Chunk16 pk[2], pv[2];
  auto fetch = [&](int kt) {
    const int k0 = kt * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = srow0 + i * 32;
      const int kr = k0 + row;
      pk[i] = *(const Chunk16*)(kb + (long)(kr < Lmax ? kr : Lmax - 1) * HD + scol);   // rows past the diagonal are masked below
      pv[i] = *(const Chunk16*)(vb + (long)row * Lp + k0 + scol);
    }
  };
  fetch(0);
  for (int kt = 0; kt <= qt; ++kt) {
    const int k0 = kt * 64;
    __syncthreads();   // every wave is done with the previous tile
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(Chunk16*)(sK + (srow0 + i * 32) * PITCHK + scol) = pk[i];
      VT::store(sV, srow0 + i * 32, tid & 7, pv[i]);
    }
    __syncthreads();
    if (kt < qt) fetch(kt + 1);
    bf16x8 kf[4][2];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const bf16_t* krow = sK + (sub * 16 + lr) * PITCHK;
      kf[sub][0] = *(const bf16x8*)(krow + lg * 8);
      kf[sub][1] = *(const bf16x8*)(krow + 32 + lg * 8);
    }
    bf16x8 vf[4][2];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) vf[d][pr] = VT::frag(sV, d * 16 + lr, pr * 4 + lg);
    f32x4 sc[4];
    float mt = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
      sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[sub][0], qf0, sc[sub], 0, 0, 0);
      sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[sub][1], qf1, sc[sub], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + sub * 16 + lg * 4 + r;
        sc[sub][r] = key <= q ? sc[sub][r] * scale : -INFINITY;
        mt = fmaxf(mt, sc[sub][r]);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);            // finite: key 0 <= q is in the first tile of every row
    const float alpha = expf(m - mn);         // first tile: exp(-inf) = 0
    m = mn;
    float ps = 0.f;
    bf16x8 pf[2];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = expf(sc[sub][r] - mn);
        ps += pv;
        pf[sub >> 1][(sub & 1) * 4 + r] = (bf16_t)pv;
      }
    lsum = lsum * alpha + ps;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[d][r] *= alpha;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[d][pr], pf[pr], o[d], 0, 0, 0);
    }
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (q < L) {
    const float inv = 1.0f / lsum;
    bf16_t* orow = out + ((long)b * L + q) * H + h * HD + lg * 4;
#pragma unroll
    for (int d = 0; d < 4; ++d)
      *(bf16x4*)(orow + d * 16) = bf16x4{(bf16_t)(o[d][0] * inv), (bf16_t)(o[d][1] * inv), (bf16_t)(o[d][2] * inv), (bf16_t)(o[d][3] * inv)};
  }
}

// qkv: [B*L][3H] with q already roped in place; kc: roped keys [B][heads][Lmax][64]; vt: V^T [B][heads][64][Lp] (finite
// beyond L); out [B*L][H].  bf16, head_dim 64 only (returns -1 otherwise: the caller keeps the three-kernel path).
int launch_flash_prefill(const void* qkv, const void* kc, const void* vt, void* out, int B, int L, int Lp, int heads, int hd, int Lmax,
                         DType dt, hipStream_t st) {
  if (dt != BF16 || hd != 64 || L <= 0 || Lp % 64 != 0 || Lp < L) return -1;
  dim3 grid((unsigned)cdiv(L, 64), (unsigned)(B * heads));
  hipLaunchKernelGGL(flash_prefill_kernel, grid, dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)kc, (const bf16_t*)vt, (bf16_t*)out, L,
                     Lp, heads, Lmax, 1.0f / sqrtf((float)hd));
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ chunk attention (ivg_kv_extend)
// T given tokens appended to a kept cache: query rows t = 0 .. T-1 of one (trajectory, head) at positions pos0 + t against keys
// [0, pos0 + t] of the cache, whose rows [pos0, pos0 + T) launch_rope_kv(pos0) has just appended.  bf16, head_dim 64.
// Workgroup = one tile of 16 * NQ query rows; its key range [0, nk), nk = pos0 + (last row of the tile) + 1, is cut into 64-key tiles and
// tile kt belongs to wave kt % 4: every K / V row is read once per query tile.  Per tile, flash_prefill_kernel's dataflow:
//   S = K Q^T      a = K rows straight from the cache, b = Q rows                          -> lane: S[key = 16 sub + 4 lg + r][q = lr]
//   online softmax in fp32 per wave (a row lives in the 4 lanes lr + 16 lg); P rounded to bf16 for P.V, the row sum keeps the fp32 P
//   O += V^T P     b = the lane's own S registers (K index of a 32-key step pr: element j = key (2 pr + j / 4) * 16 + 4 lg + j % 4)
//                  a = V^T in that key order.  V is row-major in the cache and no V^T image of past rows exists: the wave stages its
//                  tile row-major in LDS and reads it back transposed (ds_read_b64_tr_b16: the 16 lanes of group lg fetch keys
//                  (2 pr + half) * 16 + 4 lg + 0..3 x channels 16 d .. 16 d + 15, lane lr receives channel 16 d + lr of the 4 keys)
// The four waves' (max, sum, O) are merged by wave 0 in the order 0, 1, 2, 3 (LDS, no atomics).  Keys past a row's diagonal are masked
// by select; V rows >= nk are staged as zeros (they may hold NaN, and P = 0 would not silence that).  A row's result depends on
// (pos0, T, t) and its own trajectory's data only.
template <int NQ>
__global__ __launch_bounds__(256) void chunk_attn_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ kc,
                                                         const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, int T, int pos0,
                                                         int heads, int Lmax, float scale) {
  constexpr int HD = 64, QT = 16 * NQ, PITCH = HD + 8;   // staged V rows of 144 bytes: 16-byte chunks in, 8-byte transposed reads out
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / heads, h = bh - b * heads;
  const int H = heads * HD;
  const int t0 = blockIdx.x * QT;
  const int nk = pos0 + (t0 + QT < T ? t0 + QT : T);   // keys any row of this tile sees: [0, nk)
  const int ntile = (nk + 63) >> 6;
  // one buffer: the four waves' V tiles during the key loop, then the partial O of waves 1 .. 3 for the merge
  __shared__ __attribute__((aligned(16))) bf16_t sbuf[4 * 64 * PITCH];
  __shared__ float sM[4][QT], sL[4][QT];
  bf16_t* sV = sbuf + wave * 64 * PITCH;
  bf16x8 qf[NQ][2];
  int qpos[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int t = t0 + n * 16 + lr, tc = t < T ? t : T - 1;   // rows past T repeat the last one and are not stored
    qpos[n] = pos0 + tc;
    const bf16_t* qrow = qkv + ((long)b * T + tc) * 3 * H + h * HD;
    qf[n][0] = *(const bf16x8*)(qrow + lg * 8);
    qf[n][1] = *(const bf16x8*)(qrow + 32 + lg * 8);
  }
  const bf16_t* kb = kc + (long)bh * Lmax * HD;
  const bf16_t* vb = vc + (long)bh * Lmax * HD;
  f32x4 o[NQ][4];
  float m[NQ], lsum[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    m[n] = -INFINITY; lsum[n] = 0.f;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[n][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int kt = wave; kt < ntile; kt += 4) {   // (wave-uniform trip count: every lane is active at the transposed reads)
    const int k0 = kt * 64;
    bf16x8 kf[4][2];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int kr = k0 + sub * 16 + lr;
      const bf16_t* krow = kb + (long)(kr < Lmax ? kr : Lmax - 1) * HD;   // rows past the diagonal are masked below
      kf[sub][0] = *(const bf16x8*)(krow + lg * 8);
      kf[sub][1] = *(const bf16x8*)(krow + 32 + lg * 8);
    }
    Chunk16 pv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = i * 8 + (lane >> 3);
      pv[i] = k0 + row < nk ? *(const Chunk16*)(vb + (long)(k0 + row) * HD + (lane & 7) * 8) : Chunk16{0u, 0u, 0u, 0u};
    }
    __builtin_amdgcn_wave_barrier();   // the wave's transposed reads of the previous tile come before these stores
#pragma unroll
    for (int i = 0; i < 8; ++i) *(Chunk16*)(sV + (i * 8 + (lane >> 3)) * PITCH + (lane & 7) * 8) = pv[i];
    __builtin_amdgcn_wave_barrier();   // LDS operations of one wave complete in order: the reads below see every lane's stores
    bf16x8 vf[4][2];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        bf16x4 half[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const bf16_t* p = sV + ((2 * pr + hh) * 16 + 4 * lg + (lr >> 2)) * PITCH + d * 16 + 4 * (lr & 3);
          half[hh] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p));
        }
        vf[d][pr] = bf16x8{half[0][0], half[0][1], half[0][2], half[0][3], half[1][0], half[1][1], half[1][2], half[1][3]};
      }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      f32x4 sc[4];
      float mt = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
        sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[sub][0], qf[n][0], sc[sub], 0, 0, 0);
        sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[sub][1], qf[n][1], sc[sub], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + sub * 16 + lg * 4 + r;
          sc[sub][r] = key <= qpos[n] ? sc[sub][r] * scale : -INFINITY;
          mt = fmaxf(mt, sc[sub][r]);
        }
      }
      mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float mn = fmaxf(m[n], mt);
      const float ms = mn == -INFINITY ? 0.f : mn;   // a wave's tiles may all lie past an early row's diagonal: its P stays 0
      const float alpha = expf(m[n] - ms);           // first visible tile: exp(-inf) = 0
      m[n] = mn;
      float ps = 0.f;
      bf16x8 pf[2];
#pragma unroll
      for (int sub = 0; sub < 4; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pw = expf(sc[sub][r] - ms);
          ps += pw;
          pf[sub >> 1][(sub & 1) * 4 + r] = (bf16_t)pw;
        }
      lsum[n] = lsum[n] * alpha + ps;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[n][d][r] *= alpha;
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) o[n][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[d][pr], pf[pr], o[n][d], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    lsum[n] += __shfl_xor(lsum[n], 16, 64);
    lsum[n] += __shfl_xor(lsum[n], 32, 64);
    if (lg == 0) { sM[wave][n * 16 + lr] = m[n]; sL[wave][n * 16 + lr] = lsum[n]; }
  }
  __syncthreads();   // every wave is done with its V tiles
  float* sO = (float*)sbuf;   // [wave - 1][n][d][r][lane]
  if (wave > 0) {
#pragma unroll
    for (int n = 0; n < NQ; ++n)
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) sO[((((wave - 1) * NQ + n) * 4 + d) * 4 + r) * 64 + lane] = o[n][d][r];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int qi = n * 16 + lr, t = t0 + qi;
    float M = m[n];   // finite: key 0 is in tile 0, wave 0's, and every row sees it
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, sM[w][qi]);
    const float s0 = expf(m[n] - M);
    float L = lsum[n] * s0;
    f32x4 acc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[d][r] = o[n][d][r] * s0;
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float sw_ = expf(sM[w][qi] - M);   // a wave without a visible key: exp(-inf) = 0 times its zeros
      L += sL[w][qi] * sw_;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[d][r] += sO[((((w - 1) * NQ + n) * 4 + d) * 4 + r) * 64 + lane] * sw_;
    }
    if (t < T) {
      const float inv = 1.0f / L;
      bf16_t* orow = out + ((long)b * T + t) * H + h * HD + lg * 4;
#pragma unroll
      for (int d = 0; d < 4; ++d)
        *(bf16x4*)(orow + d * 16) = bf16x4{(bf16_t)(acc[d][0] * inv), (bf16_t)(acc[d][1] * inv), (bf16_t)(acc[d][2] * inv), (bf16_t)(acc[d][3] * inv)};
    }
  }
}

// qkv: [B*T][3H] with q roped in place; kc / vc: [B][heads][Lmax][64] holding positions [0, pos0 + T); out [B*T][H].  bf16, head_dim 64
// only (-1 otherwise, and for a chunk that does not fit the cache: nothing is launched)
int launch_chunk_attn(const void* qkv, const void* kc, const void* vc, void* out, int B, int T, int heads, int hd, int Lmax, int pos0,
                      DType dt, hipStream_t st) {
  if (dt != BF16 || hd != 64 || B <= 0 || heads <= 0 || T < 1 || pos0 < 0 || (long)pos0 + T > Lmax) return -1;
  if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 7) || ((uintptr_t)kc & 15) || ((uintptr_t)vc & 15)) return -1;
  const float scale = 1.0f / sqrtf((float)hd);
  if (T > 16)   // 32 query rows per workgroup: a 17-token frame reads its K / V rows once
    hipLaunchKernelGGL(chunk_attn_kernel<2>, dim3((unsigned)cdiv(T, 32), (unsigned)(B * heads)), dim3(256), 0, st, (const bf16_t*)qkv,
                       (const bf16_t*)kc, (const bf16_t*)vc, (bf16_t*)out, T, pos0, heads, Lmax, scale);
  else
    hipLaunchKernelGGL(chunk_attn_kernel<1>, dim3(1u, (unsigned)(B * heads)), dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)kc,
                       (const bf16_t*)vc, (bf16_t*)out, T, pos0, heads, Lmax, scale);
  return (int)hipGetLastError();
}

static std::atomic<long long> g_kv_extend_rows[2] = {{0}, {0}};
void kv_extend_note(int chunk_rows, int step_rows) { g_kv_extend_rows[0] += chunk_rows; g_kv_extend_rows[1] += step_rows; }
long long kv_extend_rows(int stepwise) { return g_kv_extend_rows[stepwise ? 1 : 0].load(); }
static std::atomic<long long> g_kv_extend_heads[2] = {{0}, {0}};
void kv_extend_heads_note(int frame_rows, int scored_rows) { g_kv_extend_heads[0] += frame_rows; g_kv_extend_heads[1] += scored_rows; }
long long kv_extend_heads_rows(int scored) { return g_kv_extend_heads[scored ? 1 : 0].load(); }

// ------------------------------------------------------------------------------------------------ tokenizer cross-attention
// CrossAttentionBlock's multi-head attention (ivideogpt/vq_model/conditional_vae.py:38-55) in one pass, bf16:
// every future frame's P = side^2 query tokens attend to the kv = ctx * P projected context tokens of ITS trajectory.  Replaces the
// batched score GEMM, the row softmax over an fp32 score matrix in HBM (1.9 GB at config 2) and the batched P.V GEMM.
// Same dataflow as flash_prefill_kernel (S = K Q^T, online softmax in fp32, O += V^T P with the lane's own S registers as its P
// fragment), without a mask, for head dims 128 / 192 (C = 512 / 768, four heads):
//   q   [M][P][C]   frame m = b * F + f, head h reads channels [h * HD, (h + 1) * HD)
//   Kp  [B][kv][C]  projected keys of trajectory b (shared by its F frames)
//   VpT [B][C][kv]  projected values, transposed
//   out [M][P][C]
template <int HD, int KT, bool PRE = true>   // KT: keys per staged tile (64; 32 for the single-head self-attention of 512 / 768 channels: LDS);
                                            // PRE: the next tile travels into registers under the current one (off at 768 channels: registers)
__global__ __launch_bounds__(256) void xattn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ Kp, const bf16_t* __restrict__ VpT,
                                                    bf16_t* __restrict__ out, int P, int kv, int C, int F, int nh, float scale) {
  constexpr int KQ = HD / 32;   // MFMA K-steps of the score product
  constexpr int DO = HD / 16;   // 16-row tiles of V^T / output channels
  constexpr int SUB = KT / 16;  // 16-key sub-tiles of the score tile
  constexpr int NPF = KT / 32;  // 32-key P fragments of the P.V product
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int qt = blockIdx.x;
  const int mh = blockIdx.y, m = mh / nh, h = mh - m * nh, b = m / F;
  const int qi = qt * 64 + wave * 16 + lr;               // P is a multiple of 64 (16 x 16 or 32 x 32 tokens)
  const bf16_t* qrow = q + ((long)m * P + qi) * C + h * HD;
  bf16x8 qf[KQ];
#pragma unroll
  for (int k = 0; k < KQ; ++k) qf[k] = *(const bf16x8*)(qrow + k * 32 + lg * 8);
  const bf16_t* kb = Kp + (long)b * kv * C + h * HD;     // row stride C
  const bf16_t* vb = VpT + ((long)b * C + h * HD) * kv;  // row stride kv
  f32x4 o[DO];
#pragma unroll
  for (int d = 0; d < DO; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, lsum = 0.f;
  constexpr int PK = HD + 16;   // staged K row (elements), read back as 16-byte fragments: 32 bytes of pad are conflict-free for
                                // ds_read_b128's lane groups (16 bytes cost every read a second cycle: 42 % conflict cycles in round 2)
  using VT = VtTile<KT>;        // staged V^T rows: key-permuted, one ds_read_b128 per fragment (above)
  __shared__ __attribute__((aligned(16))) bf16_t sK[KT * PK];
  __shared__ __attribute__((aligned(16))) bf16_t sV[HD * VT::PITCH];
  constexpr int KC = KT * HD / 8 / 256;   // 16-byte chunks of the K tile per thread
  constexpr int VC = HD * KT / 8 / 256;   // ... of the V^T tile
  constexpr int VCH = KT / 8;             // chunks per V^T row
  static_assert(KC >= 1 && VC >= 1, "tile too small for 256 threads");
  Chunk16 pk[KC], pvv[VC];
  auto fetch = [&](int kt) {
    const int k0 = kt * KT;
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      const int c = i * 256 + tid, row = c / (HD / 8), col = (c % (HD / 8)) * 8;
      pk[i] = *(const Chunk16*)(kb + (long)(k0 + row) * C + col);
    }
#pragma unroll
    for (int i = 0; i < VC; ++i) {
      const int c = i * 256 + tid, row = c / VCH, col = (c % VCH) * 8;
      pvv[i] = *(const Chunk16*)(vb + (long)row * kv + k0 + col);
    }
  };
  const int ntiles = kv / KT;
  if constexpr (PRE) fetch(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();   // every wave is done with the previous tile
    if constexpr (!PRE) fetch(kt);
#pragma unroll
    for (int i = 0; i < KC; ++i) { const int c = i * 256 + tid; *(Chunk16*)(sK + (c / (HD / 8)) * PK + (c % (HD / 8)) * 8) = pk[i]; }
#pragma unroll
    for (int i = 0; i < VC; ++i) { const int c = i * 256 + tid; VT::store(sV, c / VCH, c % VCH, pvv[i]); }
    __syncthreads();
    if constexpr (PRE) { if (kt + 1 < ntiles) fetch(kt + 1); }
    f32x4 sc[SUB];
    float mt = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < SUB; ++sub) {
      sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16_t* krow = sK + (sub * 16 + lr) * PK + lg * 8;
#pragma unroll
      for (int k = 0; k < KQ; ++k) sc[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(krow + k * 32), qf[k], sc[sub], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) { sc[sub][r] *= scale; mt = fmaxf(mt, sc[sub][r]); }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(mx, mt);
    const float alpha = expf(mx - mn);        // first tile: exp(-inf) = 0
    mx = mn;
    float ps = 0.f;
    bf16x8 pf[NPF];
#pragma unroll
    for (int sub = 0; sub < SUB; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pe = expf(sc[sub][r] - mn);
        ps += pe;
        pf[sub >> 1][(sub & 1) * 4 + r] = (bf16_t)pe;
      }
    lsum = lsum * alpha + ps;
#pragma unroll
    for (int d = 0; d < DO; ++d) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[d][r] *= alpha;
#pragma unroll
      for (int pr = 0; pr < NPF; ++pr)
        o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(VT::frag(sV, d * 16 + lr, pr * 4 + lg), pf[pr], o[d], 0, 0, 0);
    }
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  const float inv = 1.0f / lsum;
  bf16_t* orow = out + ((long)m * P + qi) * C + h * HD + lg * 4;
#pragma unroll
  for (int d = 0; d < DO; ++d)
    *(bf16x4*)(orow + d * 16) = bf16x4{(bf16_t)(o[d][0] * inv), (bf16_t)(o[d][1] * inv), (bf16_t)(o[d][2] * inv), (bf16_t)(o[d][3] * inv)};
}

// one predicate for the planner and the launcher: which (dtype, shape) the one-pass kernel covers
bool xattn_covers(int P, int kv, int C, int nh, DType dt) {
  if (dt != BF16 || nh <= 0 || C % nh != 0 || P % 64 != 0 || kv % 64 != 0 || (C & 7)) return false;
  const int hd = C / nh;
  return hd == 32 || hd == 64 || hd == 128 || hd == 192 || hd == 512 || hd == 768;
}

// -1: shape / dtype not covered (the caller keeps the score GEMM + softmax + P.V GEMM path)
int launch_xattn(const void* q, const void* Kp, const void* VpT, void* out, int M, int F, int P, int kv, int C, int nh, DType dt, hipStream_t st) {
  if (!xattn_covers(P, kv, C, nh, dt) || M <= 0 || F <= 0 || M % F != 0) return -1;
  if (((uintptr_t)q & 15) || ((uintptr_t)Kp & 15) || ((uintptr_t)VpT & 15) || ((uintptr_t)out & 7)) return -1;
  const int hd = C / nh;
  dim3 grid((unsigned)(P / 64), (unsigned)(M * nh));
  const float scale = 1.0f / sqrtf((float)hd);
#define IVG_XATTN(HDv, KTv, PREv) hipLaunchKernelGGL((xattn_kernel<HDv, KTv, PREv>), grid, dim3(256), 0, st, (const bf16_t*)q, (const bf16_t*)Kp, (const bf16_t*)VpT, (bf16_t*)out, P, kv, C, F, nh, scale)
  if (hd == 128) IVG_XATTN(128, 64, true);
  else if (hd == 192) IVG_XATTN(192, 64, true);
  else if (hd == 64) IVG_XATTN(64, 64, true);
  else if (hd == 32) IVG_XATTN(32, 64, true);
  else if (hd == 512) IVG_XATTN(512, 32, true);   // diffusers Attention of the conditional mid blocks: one head of 512 / 768 channels
  else if (hd == 768) IVG_XATTN(768, 32, false);
  else return -1;
#undef IVG_XATTN
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ decode attention
// One workgroup per (b, head): RoPE of the new q/k, KV-cache append and single-token attention in one launch.
// HBM-bound stream of the K and V rows of the cache (coalesced: LPK lanes share one row, 16 bytes each, four
// independent row loads in flight per lane).  Two passes over LDS-held scores -> deterministic reduction order.
// q of one lane for the key dot products: fp32 values (fp32 caches) or packed bf16 pairs (bf16 caches)
template <typename T> struct QPack;
template <> struct QPack<float> {
  __device__ __forceinline__ void set(const float*) {}
  __device__ __forceinline__ float dot(const float* qf, Chunk16 raw) const {
    const f32x4 kk = __builtin_bit_cast(f32x4, raw);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) d = fmaf(qf[j], kk[j], d);
    return d;
  }
};
template <> struct QPack<bf16_t> {
  bf16x2 q[4];
  __device__ __forceinline__ void set(const float* qf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = bf16x2{(bf16_t)qf[2 * j], (bf16_t)qf[2 * j + 1]};
  }
  __device__ __forceinline__ float dot(const float*, Chunk16 raw) const {
    const bf16x8 kk = __builtin_bit_cast(bf16x8, raw);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) d = __builtin_amdgcn_fdot2_f32_bf16(q[j], bf16x2{kk[2 * j], kk[2 * j + 1]}, d, false);
    return d;
  }
};
template <typename T> __device__ __forceinline__ float dot_chunk(const float* qf, Chunk16 raw) {
  constexpr int VEC = Traits<T>::VEC;
  float d = 0.f;
  if constexpr (sizeof(T) == 2) {
    const bf16x8 kk = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
    for (int j = 0; j < VEC; ++j) d = fmaf(qf[j], (float)kk[j], d);
  } else {
    const f32x4 kk = __builtin_bit_cast(f32x4, raw);
#pragma unroll
    for (int j = 0; j < VEC; ++j) d = fmaf(qf[j], kk[j], d);
  }
  return d;
}
template <typename T> __device__ __forceinline__ void axpy_chunk(float* of, float pw, Chunk16 raw) {
  constexpr int VEC = Traits<T>::VEC;
  if constexpr (sizeof(T) == 2) {
    const bf16x8 vv = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
    for (int j = 0; j < VEC; ++j) of[j] = fmaf(pw, (float)vv[j], of[j]);
  } else {
    const f32x4 vv = __builtin_bit_cast(f32x4, raw);
#pragma unroll
    for (int j = 0; j < VEC; ++j) of[j] = fmaf(pw, vv[j], of[j]);
  }
}

// Sum over the lpk (8 or 16) adjacent lanes that share one key row, every lane receiving the total.  DPP lane permutes
// (VALU latency) instead of __shfl_xor (ds_bpermute: an LDS round trip per step, three or four dependent ones per key row
// -- that latency, not HBM, was pacing the key pass).  Same pairing tree as the xor butterfly: bitwise the same sums.
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float group_sum(float d, int lpk) {
  if (lpk >= 2) d = dpp_add<0xB1>(d);    // quad_perm [1,0,3,2]: lane ^ 1
  if (lpk >= 4) d = dpp_add<0x4E>(d);    // quad_perm [2,3,0,1]: lane ^ 2
  if (lpk >= 8) d = dpp_add<0x141>(d);   // row_half_mirror: lane i <-> 7 - i of its 8-lane half (the other quad's total)
  if (lpk >= 16) d = dpp_add<0x140>(d);  // row_mirror: lane i <-> 15 - i (the other half's total)
  for (int o = 16; o < lpk; o <<= 1) d += __shfl_xor(d, o, 64);   // head_dim > 128 (bf16): beyond a DPP row
  return d;
}

// NT: non-temporal loads of the cache rows (streamed once per step: keep them from evicting the weights)
// HD: head dimension as a compile-time value (64 for the released transformers; 0 = generic, read from the argument) -- with it
// the lane-group reductions, the group counts and the row strides are constants instead of chains of scalar branches per chunk
// (Two value blocks in flight across the softmax statistics were built and measured slower in round 3 -- 64.3 vs 61.2 ms of
// attention per step, profiles/r03_attn_pre2_ab.txt: one block per workgroup already keeps 25 MB in flight chip-wide -- removed.)
// SHARED (round 6, shared-context rollouts: ivg_generate_shared): the G rows of a group were given ONE prompt -- predict.py's
// repeat_times samples of a clip, train_gpt.generate_multiple_times, VP2's candidate action sequences over the same two frames.  The
// prompt was prefilled once per group and its K / V rows [0, P) live ONCE, in cache row `slot = (b - row0) / G` of the chunk (the rows
// a prefill of the group's prompt wrote); a trajectory's own rows -- positions >= P: the prompt's last token, which carries the row's
// action, and everything generated -- live in its own cache row b.  The two position ranges never overlap, so no second buffer
// exists: a key row t is read from the group's cache row when t < P and from the trajectory's otherwise.  The same arithmetic in the
// same order as the un-shared kernel on the same bytes; the prefix rows use default-policy loads (the other rows of the group ask for
// the same lines: they are served from L2 / Infinity Cache instead of HBM).
// WINDOW (the default body of the bf16 head_dim-64 instances; IVG_DECODE_ATTN_WINDOW=0 under IVG_DEV=1 selects the two-buffer body):
// ONE buffer of UNR chunks as a rolling window over the rows -- chunk u of the next round is requested into the registers chunk u of
// the current round was just consumed from.  Memory returns in order, so with the round unrolled every wait is a counted vmcnt and a
// lane has UNR loads outstanding at all times (the two-buffer body: UNR to 2 x UNR, in 64 registers of row data instead of 32).  The
// key -> lane-group map, the instructions per key, the order of a lane group's value rows and everything around the two passes are
// the two-buffer body's: the outputs are bit-identical.  Half the registers: twice the waves of OTHER launches fit beside it.
template <typename T, bool NT, int HD, bool SHARED = false, bool WINDOW = false>
__global__ __launch_bounds__(256) void decode_attn_kernel(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
                                                          T* __restrict__ out, const float* __restrict__ cosT,
                                                          const float* __restrict__ sinT, int heads, int hd_arg, int Lmax,
                                                          const StepState* __restrict__ state, unsigned long long* prof,
                                                          int sh_P = 0, int sh_G = 1, int sh_row0 = 0) {
  constexpr int VEC = Traits<T>::VEC;
  const int hd = HD > 0 ? HD : hd_arg;
  constexpr int UNR = 8;   // 16-byte loads in flight per lane: 3 workgroups x 256 lanes x 8 x 16 B = 96 KiB per CU
  // measurement hook (bench.py roofline): launch window = [min start, max end] over workgroups on the 100 MHz wall clock,
  // reduced per slot here (min kept as max of the complement so that 0 = not stamped) and over slots by the host
  const unsigned long long t_start = prof ? wall_clock64() : 0ull;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lpk = hd / VEC;          // lanes per key row (8 for bf16 hd=64, 16 for fp32)
  const int gpb = 256 / lpk;         // key groups per workgroup
  float* sq = (float*)smem;          // [hd] roped q   | [hd] roped new k | [hd] new v  (values already rounded to T)
  float* sk = sq + hd;
  float* sv = sk + hd;
  float* sc = sv + hd;               // [Lmax] scores
  float* red = sc + Lmax;            // [gpb][hd] partial outputs
  __shared__ float sred[8];
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sub = tid % lpk, grp = tid / lpk;
  const int H = heads * hd, half = hd / 2;
  const float scale = rsqrtf((float)hd);
  T* kb = kc + ((long)b * heads + h) * Lmax * hd;
  T* vb = vc + ((long)b * heads + h) * Lmax * hd;
  // SHARED: byte distance from this trajectory's head base to its group's (the prefix rows t < sh_P are read there); 0 otherwise
  long sh_delta = 0;
  if constexpr (SHARED) sh_delta = ((long)((b - sh_row0) / sh_G) - b) * heads * Lmax * hd * (long)sizeof(T);
  const int step = gpb * UNR;
  // rows beyond the cached keys are not requested (on average half of the last block of 256: re-reading a clamped row instead
  // measured +1 us per launch); 32-bit byte offsets from the (wave-uniform) head base
  const unsigned lane_off = (unsigned)(sub * VEC) * (unsigned)sizeof(T);
  // `limit`: rows below it are requested.  Every call but the first passes the number of cached keys; the FIRST round of key rows goes
  // out before the step counter is even read (limit = Lmax: the rows exist in the cache buffer whatever they hold; rows >= pos are
  // never used -- the score and value passes test t < pos) -- the counter's load, a dependent memory round trip at the head of every
  // launch, then overlaps that round instead of preceding it (round 6)
  auto load_row = [&](Chunk16& dst, const T* base, int t, int limit) {
    const char* rb = (const char*)base;
    if constexpr (SHARED) rb = t < sh_P ? rb + sh_delta : rb;
    const Chunk16* src = (const Chunk16*)(rb + ((unsigned)(t * hd) * (unsigned)sizeof(T) + lane_off));
    dst = t < limit ? ((NT && !SHARED) ? __builtin_nontemporal_load(src) : *src) : Chunk16{0u, 0u, 0u, 0u};
  };
  auto load_rows = [&](Chunk16 (&dst)[UNR], const T* base, int t0, int limit) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) load_row(dst[u], base, t0 + u * gpb + grp, limit);
  };
  // WINDOW: the rows through a buffer descriptor (wave-uniform: head base, bytes below `limit`) and a 32-bit lane offset -- its range
  // check returns the zeros of rows >= limit without a branch around the load (a load under a branch cannot be waited for by
  // count), and the address is one register.  SHARED: the descriptor starts at the GROUP's head base (sh_delta <= 0: a group's slot
  // is never behind its trajectories); a trajectory's own rows lie own_off bytes above it (the launcher checks that this fits).
  const unsigned own_off = (unsigned)(-sh_delta);
  auto win_load = [&](Chunk16& dst, const T* base, int t, int limit) {
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + sh_delta), 0,
                                                        (int)(own_off + (unsigned)(limit * hd) * (unsigned)sizeof(T)), 0x00020000);
    unsigned off = (unsigned)(t * hd) * (unsigned)sizeof(T) + lane_off;
    if constexpr (SHARED) off += t < sh_P ? 0u : own_off;
    dst = __builtin_bit_cast(Chunk16, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, 0, (NT && !SHARED) ? 2 : 0));
  };
  Chunk16 cur[UNR], nxt[WINDOW ? 1 : UNR];
  // the few loads of the RoPE step go out BEFORE the first round of key rows: memory returns in order, so issued after them
  // they (and the barrier behind them) would wait for the whole 32 KiB round
  float rc = 0.f, rs = 0.f, q1 = 0.f, q2 = 0.f, k1 = 0.f, k2 = 0.f;
  T va = from_f32<T>(0.f), vb2 = from_f32<T>(0.f);
  if (tid < half) {
    const T* row = qkv + (long)b * 3 * H + h * hd;
    q1 = to_f32(row[tid]); q2 = to_f32(row[tid + half]);
    k1 = to_f32(row[H + tid]); k2 = to_f32(row[H + tid + half]);
    va = row[2 * H + tid]; vb2 = row[2 * H + tid + half];
  }
  if constexpr (WINDOW) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) win_load(cur[u], kb, u * gpb + grp, Lmax);
  } else {
    load_rows(cur, kb, 0, Lmax);  // the first key rows are in flight while the step counter arrives and q is roped
  }
  const int pos = state->pos;        // position of the token being fed = number of cached keys
  const int n_keys = pos + 1;
  if (tid < half) { rc = cosT[(long)pos * half + tid]; rs = sinT[(long)pos * half + tid]; }
  if (tid < half) {  // RoPE (HF rotate_half) of q and the new k; append k, v to the cache
    const T qa = from_f32<T>(q1 * rc - q2 * rs), qb = from_f32<T>(q2 * rc + q1 * rs);
    const T ka = from_f32<T>(k1 * rc - k2 * rs), kb2 = from_f32<T>(k2 * rc + k1 * rs);
    sq[tid] = to_f32(qa); sq[tid + half] = to_f32(qb);
    sk[tid] = to_f32(ka); sk[tid + half] = to_f32(kb2);
    sv[tid] = to_f32(va); sv[tid + half] = to_f32(vb2);
    kb[(long)pos * hd + tid] = ka; kb[(long)pos * hd + tid + half] = kb2;
    vb[(long)pos * hd + tid] = va; vb[(long)pos * hd + tid + half] = vb2;
  }
  __syncthreads();
  float qf[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) qf[j] = sq[sub * VEC + j];
  // bf16: q (already rounded to bf16) as packed pairs for v_dot2c_f32_bf16 -- two products per instruction, no unpacking of
  // the key chunk (the products are exact either way; 4 instead of 16 instructions per 16-byte chunk)
  QPack<T> qp;
  qp.set(qf);
  // pass A: scores of the cached keys (the new key comes from LDS); the next rows are requested before the current
  // ones are consumed, and the first value rows before the softmax statistics.  The two row buffers swap roles every
  // iteration (unrolled by two: no register copies); the value rows requested last end up in `cur` for pass C.
  auto scores = [&](Chunk16 (&rows)[UNR], int t0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * gpb + grp;
      float d = qp.dot(qf, rows[u]);
      d = group_sum(d, lpk);
      if (t < pos && sub == 0) sc[t] = d * scale;
    }
  };
  if constexpr (WINDOW) {
    // the window: chunk u scored, then chunk u of the next round (key rows, or the first value rows behind the last key round)
    // requested into its registers
    for (int t0 = 0; t0 < pos; t0 += step) {
      const bool more = t0 + step < pos;
      const T* nb = more ? kb : vb;
      const int nt0 = more ? t0 + step : 0;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int t = t0 + u * gpb + grp;
        float d = qp.dot(qf, cur[u]);
        d = group_sum(d, lpk);
        if (t < pos && sub == 0) sc[t] = d * scale;
        win_load(cur[u], nb, nt0 + u * gpb + grp, pos);
      }
    }
  } else {
    int t0 = 0;
    bool in_nxt = false;   // the rows to consume next are in `nxt`
    while (t0 < pos) {
      if (t0 + step < pos) load_rows(nxt, kb, t0 + step, pos); else load_rows(nxt, vb, 0, pos);
      scores(cur, t0);
      t0 += step;
      in_nxt = true;
      if (t0 >= pos) break;
      if (t0 + step < pos) load_rows(cur, kb, t0 + step, pos); else load_rows(cur, vb, 0, pos);
      scores(nxt, t0);
      t0 += step;
      in_nxt = false;
    }
    if (in_nxt) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) cur[u] = nxt[u];
    }
  }
  if (grp == 0) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) d = fmaf(qf[j], sk[sub * VEC + j], d);
    d = group_sum(d, lpk);
    if (sub == 0) sc[pos] = d * scale;
  }
  __syncthreads();
  // pass B: softmax statistics
  float mx = -INFINITY;
  for (int t = tid; t < n_keys; t += 256) mx = fmaxf(mx, sc[t]);
  mx = wave_max(mx);
  if (lane == 0) sred[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
  float sum = 0.f;
  for (int t = tid; t < n_keys; t += 256) { const float e = expf(sc[t] - mx); sc[t] = e; sum += e; }
  sum = wave_sum(sum);
  if (lane == 0) sred[4 + wv] = sum;
  __syncthreads();
  sum = (sred[4] + sred[5]) + (sred[6] + sred[7]);
  // pass C: weighted V sum; group `grp` takes keys grp, grp+gpb, ... (fixed order), the new token's v from LDS
  float of[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) of[j] = 0.f;
  auto weighted = [&](Chunk16 (&rows)[UNR], int t0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * gpb + grp;
      if (t < pos) axpy_chunk<T>(of, sc[t], rows[u]);
    }
  };
  if constexpr (WINDOW) {   // cur holds value rows [0, step); every round but the last refills the window behind itself
    int t0 = 0;
    for (; t0 + step < pos; t0 += step) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int t = t0 + u * gpb + grp;
        axpy_chunk<T>(of, sc[t], cur[u]);   // t < t0 + step < pos
        // a straight-line round: the sums pinned here and the scheduler fenced below, or the optimiser regroups the round's
        // multiply-adds by output element behind all of its requests -- into a second buffer of registers
#pragma unroll
        for (int j = 0; j < VEC; ++j) asm volatile("" : "+v"(of[j]));
        win_load(cur[u], vb, t + step, pos);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (pos > 0) weighted(cur, t0);
  } else {
    for (int t0 = 0; t0 < pos; t0 += 2 * step) {  // cur holds value rows [t0, t0 + step) (requested during pass A / the last iteration)
      if (t0 + step < pos) load_rows(nxt, vb, t0 + step, pos);
      weighted(cur, t0);
      if (t0 + step >= pos) break;
      if (t0 + 2 * step < pos) load_rows(cur, vb, t0 + 2 * step, pos);
      weighted(nxt, t0 + step);
    }
  }
  if (grp == 0) {
    const float pw = sc[pos];
#pragma unroll
    for (int j = 0; j < VEC; ++j) of[j] = fmaf(pw, sv[sub * VEC + j], of[j]);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) red[grp * hd + sub * VEC + j] = of[j];
  __syncthreads();
  if (tid < hd) {
    float a = 0.f;
    for (int g = 0; g < gpb; ++g) a += red[g * hd + tid];
    out[(long)b * H + h * hd + tid] = from_f32<T>(a / sum);
  }
  if (prof && tid == 0) {
    unsigned long long* slot = prof + (size_t)((blockIdx.x * 7 + blockIdx.y) % IVG_ATTN_PROF_SLOTS) * 2 * Lmax;
    atomicMax(slot + pos, ~t_start);
    atomicMax(slot + Lmax + pos, (unsigned long long)wall_clock64());
  }
}

bool decode_attn_covers(int hd, DType dt) {
  const int vec = dt == BF16 ? 8 : 4;
  return hd > 0 && hd <= 256 && hd % vec == 0 && 256 % (hd / vec) == 0;
}

int launch_decode_attn(const void* qkv, void* kc, void* vc, void* out, const float* cosT, const float* sinT, int B, int heads, int hd,
                       int Lmax, const StepState* state, unsigned long long* prof, DType dt, hipStream_t st, int sh_P, int sh_G, int sh_row0) {
  if (!decode_attn_covers(hd, dt)) return (int)hipErrorInvalidValue;
  const int vec = dt == BF16 ? 8 : 4;
  const int gpb = 256 / (hd / vec);
  const size_t smem = (size_t)(3 * hd + Lmax + gpb * hd) * sizeof(float);
  dim3 g(B * heads);
  const bool window = sw().decode_attn_window != 0;   // bf16, head_dim 64: the rolling-window body (development switch: the two-buffer one)
  // non-temporal cache-row loads (bf16): 5.57 -> 6.28 TB/s on a pure stream, 203 -> 191 ms per rollout
#define IVG_DA(T, NTv, HDv) \
  hipLaunchKernelGGL((decode_attn_kernel<T, NTv, HDv>), g, dim3(256), smem, st, (const T*)qkv, (T*)kc, (T*)vc, (T*)out, cosT, sinT, heads, hd, Lmax, state, prof, 0, 1, 0)
  if (sh_G > 1) {   // shared-context rollout: prefix rows from the group's cache row
    if (sh_P < 0 || sh_row0 > 0) return (int)hipErrorInvalidValue;
#define IVG_DAS(T, NTv, HDv) \
  hipLaunchKernelGGL((decode_attn_kernel<T, NTv, HDv, true>), g, dim3(256), smem, st, (const T*)qkv, (T*)kc, (T*)vc, (T*)out, cosT, sinT, heads, hd, Lmax, state, prof, sh_P, sh_G, sh_row0)
    // the window body addresses a trajectory's rows from its GROUP's head base: the slot not behind the row, 32-bit distances
    const bool near = sh_row0 > -sh_G && (long)B * heads * Lmax * hd * 2 < (1l << 32);
    if (dt == BF16 && hd == 64 && window && near)
      hipLaunchKernelGGL((decode_attn_kernel<bf16_t, true, 64, true, true>), g, dim3(256), smem, st, (const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (bf16_t*)out, cosT, sinT, heads, hd, Lmax, state, prof, sh_P, sh_G, sh_row0);
    else if (dt == BF16) { if (hd == 64) IVG_DAS(bf16_t, true, 64); else IVG_DAS(bf16_t, true, 0); }
    else { if (hd == 64) IVG_DAS(float, false, 64); else IVG_DAS(float, false, 0); }
#undef IVG_DAS
    return (int)hipGetLastError();
  }
  if (dt == BF16 && hd == 64 && window)
    hipLaunchKernelGGL((decode_attn_kernel<bf16_t, true, 64, false, true>), g, dim3(256), smem, st, (const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (bf16_t*)out, cosT, sinT, heads, hd, Lmax, state, prof, 0, 1, 0);
  else if (dt == BF16) { if (hd == 64) IVG_DA(bf16_t, true, 64); else IVG_DA(bf16_t, true, 0); }
  else { if (hd == 64) IVG_DA(float, false, 64); else IVG_DA(float, false, 0); }
#undef IVG_DA
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 24-bit K / V cache of the x3 rollout
// The 1e-3-compliant rollout mode (IVG_F32X3) keeps fp32 tensors, and its decode attention streamed an fp32 cache: 249 MB per layer
// and step at config 2, 130 of the mode's 425 ms per step (45.8 us per launch; over the planes below: 32.8 us, 93 ms).  The arithmetic of that mode carries 2^-17 per operand anyway (bf16 hi +
// bf16 lo), so the cache keeps 24 of the 32 bits: sign, exponent and 15 mantissa bits, rounded to nearest even -- 2^-17 relative --
// as TWO PLANES per (trajectory, head): the upper 16 bits of every element ([Lmax][64] uint16, a bf16 image of the row) followed by
// the next 8 bits ([Lmax][64] uint8).  A key row is 128 + 64 bytes instead of 256; a lane reads 16 + 8 bytes (8 elements) and
// rebuilds each fp32 value with one v_perm_b32.  Everything else is decode_attn_kernel's structure (8 lanes per key row, as its bf16
// instance): first round of key rows before the step counter, scores -> LDS, softmax statistics, weighted value sum in fixed order.
// The appended k / v are rounded BEFORE they are used for this step's own score and output, so a later step reads exactly what
// this one computed with.  The prefill keeps fp32 K / V of one layer in scratch (its score GEMM reads K as a matrix) and packs the
// rows into the planes afterwards (kv24_pack_kernel).
__device__ __forceinline__ unsigned f24_round(float x) {   // fp32 bits rounded to 24 (RNE), low byte zero
  unsigned u = __float_as_uint(x);
  u += 0x7fu + ((u >> 8) & 1u);
  return u & 0xffffff00u;
}
struct Row24 { Chunk16 hi; unsigned lo0, lo1; };
__device__ __forceinline__ void row24_unpack(const Row24& r, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned h = r.hi[j >> 1];
    const unsigned l = j < 4 ? r.lo0 : r.lo1;
    // result bytes: [0] = 0, [1] = byte (j & 3) of the low plane's dword, [2..3] = the element's 16 upper bits
    const unsigned sel = (j & 1) ? (0x07060000u | ((unsigned)(j & 3) << 8) | 0x0cu) : (0x05040000u | ((unsigned)(j & 3) << 8) | 0x0cu);
    f[j] = __uint_as_float(__builtin_amdgcn_perm(h, l, sel));
  }
}

template <bool SHARED>
__global__ __launch_bounds__(256) void decode_attn24_kernel(const float* __restrict__ qkv, unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                            float* __restrict__ out, const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                            int heads, int Lmax, const StepState* __restrict__ state, unsigned long long* prof,
                                                            int sh_P, int sh_G, int sh_row0) {
  constexpr int HD = 64, HALF = 32, LPK = 8, GPB = 32, UNR = 8;
  const unsigned long long t_start = prof ? wall_clock64() : 0ull;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sq = (float*)smem;
  float* sk = sq + HD;
  float* sv = sk + HD;
  float* sc = sv + HD;               // [Lmax] scores
  float* red = sc + Lmax;            // [GPB][HD] partial outputs
  __shared__ float sred[8];
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sub = tid % LPK, grp = tid / LPK;
  const int H = heads * HD;
  const float scale = rsqrtf((float)HD);
  const long blk = (long)Lmax * (HD * 3);                          // bytes of one (trajectory, head): [Lmax][64] u16 | [Lmax][64] u8
  unsigned char* kb = kc + ((long)b * heads + h) * blk;
  unsigned char* vb = vc + ((long)b * heads + h) * blk;
  const unsigned lo_plane = (unsigned)Lmax * (HD * 2);
  long sh_delta = 0;
  if constexpr (SHARED) sh_delta = ((long)((b - sh_row0) / sh_G) - b) * heads * blk;
  const int step = GPB * UNR;
  auto load_rows = [&](Row24 (&dst)[UNR], const unsigned char* base, int t0, int limit) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * GPB + grp;
      const unsigned char* rb = base;
      if constexpr (SHARED) rb = t < sh_P ? base + sh_delta : base;
      const Chunk16* ph = (const Chunk16*)(rb + ((unsigned)t * (HD * 2) + (unsigned)sub * 16u));
      typedef unsigned int U2 __attribute__((ext_vector_type(2)));
      const U2* pl = (const U2*)(rb + (lo_plane + (unsigned)t * HD + (unsigned)sub * 8u));
      if (t < limit) {
        if constexpr (SHARED) { dst[u].hi = *ph; const U2 l2 = *pl; dst[u].lo0 = l2[0]; dst[u].lo1 = l2[1]; }
        else { dst[u].hi = __builtin_nontemporal_load(ph); const U2 l2 = __builtin_nontemporal_load(pl); dst[u].lo0 = l2[0]; dst[u].lo1 = l2[1]; }
      } else {
        dst[u].hi = Chunk16{0u, 0u, 0u, 0u}; dst[u].lo0 = 0u; dst[u].lo1 = 0u;
      }
    }
  };
  Row24 cur[UNR], nxt[UNR];
  float rc = 0.f, rs = 0.f, q1 = 0.f, q2 = 0.f, k1 = 0.f, k2 = 0.f, va = 0.f, vb2 = 0.f;
  if (tid < HALF) {
    const float* row = qkv + (long)b * 3 * H + h * HD;
    q1 = row[tid]; q2 = row[tid + HALF];
    k1 = row[H + tid]; k2 = row[H + tid + HALF];
    va = row[2 * H + tid]; vb2 = row[2 * H + tid + HALF];
  }
  load_rows(cur, kb, 0, Lmax);       // the first key rows are in flight while the step counter arrives and q is roped
  const int pos = state->pos;
  const int n_keys = pos + 1;
  if (tid < HALF) { rc = cosT[(long)pos * HALF + tid]; rs = sinT[(long)pos * HALF + tid]; }
  if (tid < HALF) {
    const unsigned ka = f24_round(k1 * rc - k2 * rs), kb2 = f24_round(k2 * rc + k1 * rs);
    const unsigned v1 = f24_round(va), v2 = f24_round(vb2);
    sq[tid] = q1 * rc - q2 * rs; sq[tid + HALF] = q2 * rc + q1 * rs;
    sk[tid] = __uint_as_float(ka); sk[tid + HALF] = __uint_as_float(kb2);
    sv[tid] = __uint_as_float(v1); sv[tid + HALF] = __uint_as_float(v2);
    unsigned short* kh = (unsigned short*)kb + (long)pos * HD;
    unsigned short* vh = (unsigned short*)vb + (long)pos * HD;
    unsigned char* kl = kb + lo_plane + (long)pos * HD;
    unsigned char* vl = vb + lo_plane + (long)pos * HD;
    kh[tid] = (unsigned short)(ka >> 16); kh[tid + HALF] = (unsigned short)(kb2 >> 16);
    kl[tid] = (unsigned char)(ka >> 8); kl[tid + HALF] = (unsigned char)(kb2 >> 8);
    vh[tid] = (unsigned short)(v1 >> 16); vh[tid + HALF] = (unsigned short)(v2 >> 16);
    vl[tid] = (unsigned char)(v1 >> 8); vl[tid + HALF] = (unsigned char)(v2 >> 8);
  }
  __syncthreads();
  float qf[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) qf[j] = sq[sub * 8 + j];
  auto scores = [&](Row24 (&rows)[UNR], int t0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * GPB + grp;
      float kf[8];
      row24_unpack(rows[u], kf);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d = fmaf(qf[j], kf[j], d);
      d = group_sum(d, LPK);
      if (t < pos && sub == 0) sc[t] = d * scale;
    }
  };
  {
    int t0 = 0;
    bool in_nxt = false;
    while (t0 < pos) {
      if (t0 + step < pos) load_rows(nxt, kb, t0 + step, pos); else load_rows(nxt, vb, 0, pos);
      scores(cur, t0);
      t0 += step;
      in_nxt = true;
      if (t0 >= pos) break;
      if (t0 + step < pos) load_rows(cur, kb, t0 + step, pos); else load_rows(cur, vb, 0, pos);
      scores(nxt, t0);
      t0 += step;
      in_nxt = false;
    }
    if (in_nxt) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) cur[u] = nxt[u];
    }
  }
  if (grp == 0) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d = fmaf(qf[j], sk[sub * 8 + j], d);
    d = group_sum(d, LPK);
    if (sub == 0) sc[pos] = d * scale;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int t = tid; t < n_keys; t += 256) mx = fmaxf(mx, sc[t]);
  mx = wave_max(mx);
  if (lane == 0) sred[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
  float sum = 0.f;
  for (int t = tid; t < n_keys; t += 256) { const float e = expf(sc[t] - mx); sc[t] = e; sum += e; }
  sum = wave_sum(sum);
  if (lane == 0) sred[4 + wv] = sum;
  __syncthreads();
  sum = (sred[4] + sred[5]) + (sred[6] + sred[7]);
  float of[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) of[j] = 0.f;
  auto weighted = [&](Row24 (&rows)[UNR], int t0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * GPB + grp;
      if (t < pos) {
        float vf[8];
        row24_unpack(rows[u], vf);
        const float pw = sc[t];
#pragma unroll
        for (int j = 0; j < 8; ++j) of[j] = fmaf(pw, vf[j], of[j]);
      }
    }
  };
  for (int t0 = 0; t0 < pos; t0 += 2 * step) {
    if (t0 + step < pos) load_rows(nxt, vb, t0 + step, pos);
    weighted(cur, t0);
    if (t0 + step >= pos) break;
    if (t0 + 2 * step < pos) load_rows(cur, vb, t0 + 2 * step, pos);
    weighted(nxt, t0 + step);
  }
  if (grp == 0) {
    const float pw = sc[pos];
#pragma unroll
    for (int j = 0; j < 8; ++j) of[j] = fmaf(pw, sv[sub * 8 + j], of[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[grp * HD + sub * 8 + j] = of[j];
  __syncthreads();
  if (tid < HD) {
    float a = 0.f;
    for (int g = 0; g < GPB; ++g) a += red[g * HD + tid];
    out[(long)b * H + h * HD + tid] = a / sum;
  }
  if (prof && tid == 0) {
    unsigned long long* slot = prof + (size_t)((blockIdx.x * 7 + blockIdx.y) % IVG_ATTN_PROF_SLOTS) * 2 * Lmax;
    atomicMax(slot + pos, ~t_start);
    atomicMax(slot + Lmax + pos, (unsigned long long)wall_clock64());
  }
}

static std::atomic<long long> g_attn24_launches{0};
long long decode_attn24_launches() { return g_attn24_launches.load(); }

int launch_decode_attn24(const void* qkv, void* kc, void* vc, void* out, const float* cosT, const float* sinT, int B, int heads, int Lmax,
                         const StepState* state, unsigned long long* prof, hipStream_t st, int sh_P, int sh_G, int sh_row0) {
  g_attn24_launches.fetch_add(1, std::memory_order_relaxed);
  const size_t smem = (size_t)(3 * 64 + Lmax + 32 * 64) * sizeof(float);
  dim3 g(B * heads);
  if (sh_G > 1) {
    if (sh_P < 0 || sh_row0 > 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_attn24_kernel<true>, g, dim3(256), smem, st, (const float*)qkv, (unsigned char*)kc, (unsigned char*)vc, (float*)out, cosT, sinT,
                       heads, Lmax, state, prof, sh_P, sh_G, sh_row0);
  } else {
    hipLaunchKernelGGL(decode_attn24_kernel<false>, g, dim3(256), smem, st, (const float*)qkv, (unsigned char*)kc, (unsigned char*)vc, (float*)out, cosT, sinT,
                       heads, Lmax, state, prof, 0, 1, 0);
  }
  return (int)hipGetLastError();
}

// fp32 rows [0, L) of K / V ([B * heads][Lmax][64], what rope_kv wrote for the prompt) -> the 24-bit planes of the cache
__global__ __launch_bounds__(256) void kv24_pack_kernel(const float* __restrict__ k32, const float* __restrict__ v32, unsigned char* __restrict__ kc,
                                                        unsigned char* __restrict__ vc, int L, int Lmax) {
  const int bh = blockIdx.y, tid = threadIdx.x;
  const int row = blockIdx.x * 32 + (tid >> 3), sub = tid & 7;
  if (row >= L) return;
  const long blk = (long)Lmax * 192;
  const unsigned lo_plane = (unsigned)Lmax * 128u;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const float* src = (which ? v32 : k32) + ((long)bh * Lmax + row) * 64 + sub * 8;
    unsigned char* dst = (which ? vc : kc) + (long)bh * blk;
    const f32x4 a = *(const f32x4*)src, c = *(const f32x4*)(src + 4);
    unsigned u[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { u[j] = f24_round(a[j]); u[4 + j] = f24_round(c[j]); }
    Chunk16 hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) hi[j] = (u[2 * j] >> 16) | (u[2 * j + 1] & 0xffff0000u);
    uint2 lo;
    lo.x = ((u[0] >> 8) & 0xffu) | (u[1] & 0xff00u) | ((u[2] << 8) & 0xff0000u) | ((u[3] << 16) & 0xff000000u);
    lo.y = ((u[4] >> 8) & 0xffu) | (u[5] & 0xff00u) | ((u[6] << 8) & 0xff0000u) | ((u[7] << 16) & 0xff000000u);
    *(Chunk16*)(dst + (unsigned)row * 128u + (unsigned)sub * 16u) = hi;
    *(uint2*)(dst + lo_plane + (unsigned)row * 64u + (unsigned)sub * 8u) = lo;
  }
}

int launch_kv24_pack(const void* k32, const void* v32, void* kc, void* vc, int BH, int L, int Lmax, hipStream_t st) {
  if (L <= 0) return 0;
  hipLaunchKernelGGL(kv24_pack_kernel, dim3((unsigned)cdiv(L, 32), (unsigned)BH), dim3(256), 0, st, (const float*)k32, (const float*)v32, (unsigned char*)kc,
                     (unsigned char*)vc, L, Lmax);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ FP8 (e4m3) K / V cache of the bf16 rollout
// Opt-in (ivg_set_kv_format, include/ivg.h has the contract): the bf16 rollout keeps one byte per cache element instead of two --
// OCP e4m3fn, gfx950's native FP8 -- byte = e4m3_rne(clamp(x_bf16 / scale, -448, 448)) with x_bf16 the value the bf16 cache holds and
// `scale` a per-engine power of two (one for K, one for V).  The clamp is explicit (the conversion's overflow mode is a register
// state this code does not own) and lets NaN through: a finite value never becomes NaN, NaN stores a NaN code.  A key row is 64
// bytes: FOUR lanes share it with one 16-byte load each (the same bytes per request and requests in flight as the bf16 instance of
// decode_attn_kernel; 64 key groups per workgroup, 512 rows per round), decoded with v_cvt_pk_f32_fp8.  bf16 x e4m3 products are
// exact in fp32.  Everything else is decode_attn_kernel's structure: first round of key rows before the step counter, scores ->
// LDS, softmax statistics, weighted value sum in fixed order, SHARED row selection, stamps.  k_scale folds into the score scale,
// v_scale into the final division.  As in decode_attn24_kernel the fed k / v are rounded -- to bf16, then to e4m3 -- BEFORE they
// are used for this step's own score and output: a later step reads exactly what this one computed with.  The prompt pass keeps
// bf16 K / V of one layer in scratch and packs the rows afterwards (kv8_pack_kernel).
// Per-head scales (ivg_set_kv_scales): ks_tab / vs_tab are this layer's [heads] tables; a workgroup serves one (b, h) and reads its
// two scales once, uniformly, where the scalars are used -- null pointers mean the scalar arguments, and that path computes what it
// computed before the tables existed.  Resources with the two pointer arguments (-Rpass-analysis=kernel-resource-usage, gfx950):
// 123 VGPRs plain / 133 SHARED, occupancy 4 / 3, scratch 0 -- the figures of the kernel without them.
__device__ __forceinline__ float e4m3_clamp(float x) {
  const float c = fminf(fmaxf(x, -448.f), 448.f);
  return (__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u ? x : c;   // (fmin / fmax drop a NaN operand)
}
// a -> byte 0, b -> byte 1 of the selected half of `old` (v_cvt_pk_fp8_f32, RNE)
template <bool HI> __device__ __forceinline__ int e4m3_pair(float a, float b, int old) {
  return __builtin_amdgcn_cvt_pk_fp8_f32(e4m3_clamp(a), e4m3_clamp(b), old, HI);
}
__device__ __forceinline__ void row8_unpack(const Chunk16& r, float (&f)[16]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[w], true);
    f[4 * w] = lo[0]; f[4 * w + 1] = lo[1]; f[4 * w + 2] = hi[0]; f[4 * w + 3] = hi[1];
  }
}

constexpr int KV8_LPK = 4, KV8_GPB = 256 / KV8_LPK, KV8_UNR = 8;   // lanes per key row, key groups per workgroup, rows in flight per lane

template <bool SHARED>
__global__ __launch_bounds__(256) void decode_attn8_kernel(const bf16_t* __restrict__ qkv, unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                           bf16_t* __restrict__ out, const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                           int heads, int Lmax, const StepState* __restrict__ state, unsigned long long* prof,
                                                           float k_scale, float v_scale, int sh_P, int sh_G, int sh_row0,
                                                           const float* __restrict__ ks_tab, const float* __restrict__ vs_tab) {
  constexpr int HD = 64, HALF = 32, LPK = KV8_LPK, GPB = KV8_GPB, UNR = KV8_UNR, VEC = 16;
  const unsigned long long t_start = prof ? wall_clock64() : 0ull;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sq = (float*)smem;          // [64] roped q (bf16 values) | [64] fed k | [64] fed v, both as decoded from their e4m3 codes
  float* sk = sq + HD;
  float* sv = sk + HD;
  float* sc = sv + HD;               // [Lmax] scores
  float* red = sc + Lmax;            // [GPB][HD] partial outputs
  __shared__ float sred[8];
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sub = tid % LPK, grp = tid / LPK;
  const int H = heads * HD;
  // per-head scales (ivg_set_kv_scales): one uniform read per workgroup from this layer's [heads] tables; null: the scalar arguments
  if (ks_tab) { k_scale = ks_tab[h]; v_scale = vs_tab[h]; }
  const float scale = 0.125f * k_scale;                            // 1 / sqrt(64), and the keys' scale: both powers of two
  const float inv_ks = 1.0f / k_scale, inv_vs = 1.0f / v_scale;    // exact (kv8_scale_ok)
  const long blk = (long)Lmax * HD;                                // bytes of one (trajectory, head)
  unsigned char* kb = kc + ((long)b * heads + h) * blk;
  unsigned char* vb = vc + ((long)b * heads + h) * blk;
  long sh_delta = 0;
  if constexpr (SHARED) sh_delta = ((long)((b - sh_row0) / sh_G) - b) * heads * blk;
  const int step = GPB * UNR;
  auto load_rows = [&](Chunk16 (&dst)[UNR], const unsigned char* base, int t0, int limit) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * GPB + grp;
      const unsigned char* rb = base;
      if constexpr (SHARED) rb = t < sh_P ? base + sh_delta : base;
      const Chunk16* src = (const Chunk16*)(rb + ((unsigned)t * HD + (unsigned)sub * 16u));
      dst[u] = t < limit ? (SHARED ? *src : __builtin_nontemporal_load(src)) : Chunk16{0u, 0u, 0u, 0u};
    }
  };
  Chunk16 cur[UNR], nxt[UNR];
  float rc = 0.f, rs = 0.f, q1 = 0.f, q2 = 0.f, k1 = 0.f, k2 = 0.f, va = 0.f, vb2 = 0.f;
  if (tid < HALF) {
    const bf16_t* row = qkv + (long)b * 3 * H + h * HD;
    q1 = (float)row[tid]; q2 = (float)row[tid + HALF];
    k1 = (float)row[H + tid]; k2 = (float)row[H + tid + HALF];
    va = (float)row[2 * H + tid]; vb2 = (float)row[2 * H + tid + HALF];
  }
  load_rows(cur, kb, 0, Lmax);       // the first key rows are in flight while the step counter arrives and q is roped
  const int pos = state->pos;
  const int n_keys = pos + 1;
  if (tid < HALF) { rc = cosT[(long)pos * HALF + tid]; rs = sinT[(long)pos * HALF + tid]; }
  if (tid < HALF) {   // RoPE as decode_attn_kernel<bf16_t>; the fed k / v: bf16, then e4m3 -- used below as decoded from the stored codes
    const bf16_t qa = (bf16_t)(q1 * rc - q2 * rs), qb = (bf16_t)(q2 * rc + q1 * rs);
    const bf16_t ka = (bf16_t)(k1 * rc - k2 * rs), kb2 = (bf16_t)(k2 * rc + k1 * rs);
    const int kp = e4m3_pair<false>((float)ka * inv_ks, (float)kb2 * inv_ks, 0);
    const int vp = e4m3_pair<false>(va * inv_vs, vb2 * inv_vs, 0);
    const f32x2 kd = __builtin_amdgcn_cvt_pk_f32_fp8(kp, false), vd = __builtin_amdgcn_cvt_pk_f32_fp8(vp, false);
    sq[tid] = (float)qa; sq[tid + HALF] = (float)qb;
    sk[tid] = kd[0]; sk[tid + HALF] = kd[1];
    sv[tid] = vd[0]; sv[tid + HALF] = vd[1];
    kb[(long)pos * HD + tid] = (unsigned char)(kp & 0xff); kb[(long)pos * HD + tid + HALF] = (unsigned char)((kp >> 8) & 0xff);
    vb[(long)pos * HD + tid] = (unsigned char)(vp & 0xff); vb[(long)pos * HD + tid + HALF] = (unsigned char)((vp >> 8) & 0xff);
  }
  __syncthreads();
  float qf[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) qf[j] = sq[sub * VEC + j];
  auto scores = [&](Chunk16 (&rows)[UNR], int t0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * GPB + grp;
      float kf[VEC];
      row8_unpack(rows[u], kf);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < VEC; ++j) d = fmaf(qf[j], kf[j], d);
      d = group_sum(d, LPK);
      if (t < pos && sub == 0) sc[t] = d * scale;
    }
  };
  {
    int t0 = 0;
    bool in_nxt = false;
    while (t0 < pos) {
      if (t0 + step < pos) load_rows(nxt, kb, t0 + step, pos); else load_rows(nxt, vb, 0, pos);
      scores(cur, t0);
      t0 += step;
      in_nxt = true;
      if (t0 >= pos) break;
      if (t0 + step < pos) load_rows(cur, kb, t0 + step, pos); else load_rows(cur, vb, 0, pos);
      scores(nxt, t0);
      t0 += step;
      in_nxt = false;
    }
    if (in_nxt) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) cur[u] = nxt[u];
    }
  }
  if (grp == 0) {
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) d = fmaf(qf[j], sk[sub * VEC + j], d);
    d = group_sum(d, LPK);
    if (sub == 0) sc[pos] = d * scale;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int t = tid; t < n_keys; t += 256) mx = fmaxf(mx, sc[t]);
  mx = wave_max(mx);
  if (lane == 0) sred[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
  float sum = 0.f;
  for (int t = tid; t < n_keys; t += 256) { const float e = expf(sc[t] - mx); sc[t] = e; sum += e; }
  sum = wave_sum(sum);
  if (lane == 0) sred[4 + wv] = sum;
  __syncthreads();
  sum = (sred[4] + sred[5]) + (sred[6] + sred[7]);
  float of[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) of[j] = 0.f;
  auto weighted = [&](Chunk16 (&rows)[UNR], int t0) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = t0 + u * GPB + grp;
      if (t < pos) {
        float vf[VEC];
        row8_unpack(rows[u], vf);
        const float pw = sc[t];
#pragma unroll
        for (int j = 0; j < VEC; ++j) of[j] = fmaf(pw, vf[j], of[j]);
      }
    }
  };
  for (int t0 = 0; t0 < pos; t0 += 2 * step) {
    if (t0 + step < pos) load_rows(nxt, vb, t0 + step, pos);
    weighted(cur, t0);
    if (t0 + step >= pos) break;
    if (t0 + 2 * step < pos) load_rows(cur, vb, t0 + 2 * step, pos);
    weighted(nxt, t0 + step);
  }
  if (grp == 0) {
    const float pw = sc[pos];
#pragma unroll
    for (int j = 0; j < VEC; ++j) of[j] = fmaf(pw, sv[sub * VEC + j], of[j]);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) red[grp * HD + sub * VEC + j] = of[j];
  __syncthreads();
  if (tid < HD) {
    float a = 0.f;
    for (int g = 0; g < GPB; ++g) a += red[g * HD + tid];
    out[(long)b * H + h * HD + tid] = (bf16_t)(a / sum * v_scale);   // (the product with a power of two is exact)
  }
  if (prof && tid == 0) {
    unsigned long long* slot = prof + (size_t)((blockIdx.x * 7 + blockIdx.y) % IVG_ATTN_PROF_SLOTS) * 2 * Lmax;
    atomicMax(slot + pos, ~t_start);
    atomicMax(slot + Lmax + pos, (unsigned long long)wall_clock64());
  }
}

bool kv8_scale_ok(float s) {
  int ex = 0;
  return std::isnormal(s) && s > 0.f && frexpf(s, &ex) == 0.5f && std::isnormal(1.0f / s);
}

static std::atomic<long long> g_attn8_launches{0};
long long decode_attn8_launches() { return g_attn8_launches.load(); }

int launch_decode_attn8(const void* qkv, void* kc, void* vc, void* out, const float* cosT, const float* sinT, int B, int heads, int Lmax,
                        const StepState* state, unsigned long long* prof, float k_scale, float v_scale, hipStream_t st, int sh_P, int sh_G,
                        int sh_row0, const float* k_scales, const float* v_scales) {
  if (!kv8_scale_ok(k_scale) || !kv8_scale_ok(v_scale) || (k_scales == nullptr) != (v_scales == nullptr)) return (int)hipErrorInvalidValue;
  const size_t smem = (size_t)(3 * 64 + Lmax + KV8_GPB * 64) * sizeof(float);
  dim3 g(B * heads);
  if (sh_G > 1) {
    if (sh_P < 0 || sh_row0 > 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(decode_attn8_kernel<true>, g, dim3(256), smem, st, (const bf16_t*)qkv, (unsigned char*)kc, (unsigned char*)vc, (bf16_t*)out, cosT,
                       sinT, heads, Lmax, state, prof, k_scale, v_scale, sh_P, sh_G, sh_row0, k_scales, v_scales);
  } else {
    hipLaunchKernelGGL(decode_attn8_kernel<false>, g, dim3(256), smem, st, (const bf16_t*)qkv, (unsigned char*)kc, (unsigned char*)vc, (bf16_t*)out, cosT,
                       sinT, heads, Lmax, state, prof, k_scale, v_scale, 0, 1, 0, k_scales, v_scales);
  }
  g_attn8_launches.fetch_add(1, std::memory_order_relaxed);
  return (int)hipGetLastError();
}

// bf16 rows [0, L) of K / V ([B * heads][Lmax][64], what rope_kv wrote for the prompt into scratch) -> the byte rows of the cache.
// Never in place: byte row t overlaps bf16 row t / 2 of the same block.
__global__ __launch_bounds__(256) void kv8_pack_kernel(const bf16_t* __restrict__ k16, const bf16_t* __restrict__ v16, unsigned char* __restrict__ kc,
                                                       unsigned char* __restrict__ vc, int L, int Lmax, float inv_ks, float inv_vs, int heads,
                                                       const float* __restrict__ ks_tab, const float* __restrict__ vs_tab) {
  const int bh = blockIdx.y, tid = threadIdx.x;
  if (ks_tab) { inv_ks = 1.0f / ks_tab[bh % heads]; inv_vs = 1.0f / vs_tab[bh % heads]; }   // per-head scales: exact reciprocals of powers of two
  const int row = blockIdx.x * 32 + (tid >> 3), sub = tid & 7;
  if (row >= L) return;
  const long off = ((long)bh * Lmax + row) * 64 + sub * 8;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const bf16x8 x = *(const bf16x8*)((which ? v16 : k16) + off);
    const float inv = which ? inv_vs : inv_ks;
    int lo = e4m3_pair<false>((float)x[0] * inv, (float)x[1] * inv, 0), hi = e4m3_pair<false>((float)x[4] * inv, (float)x[5] * inv, 0);
    lo = e4m3_pair<true>((float)x[2] * inv, (float)x[3] * inv, lo);
    hi = e4m3_pair<true>((float)x[6] * inv, (float)x[7] * inv, hi);
    *(uint2*)((which ? vc : kc) + off) = uint2{(unsigned)lo, (unsigned)hi};
  }
}

int launch_kv8_pack(const void* k16, const void* v16, void* kc, void* vc, int BH, int L, int Lmax, float k_scale, float v_scale, hipStream_t st,
                    int heads, const float* k_scales, const float* v_scales) {
  if (!kv8_scale_ok(k_scale) || !kv8_scale_ok(v_scale) || heads <= 0 || (k_scales == nullptr) != (v_scales == nullptr)) return (int)hipErrorInvalidValue;
  if (L <= 0) return 0;
  hipLaunchKernelGGL(kv8_pack_kernel, dim3((unsigned)cdiv(L, 32), (unsigned)BH), dim3(256), 0, st, (const bf16_t*)k16, (const bf16_t*)v16,
                     (unsigned char*)kc, (unsigned char*)vc, L, Lmax, 1.0f / k_scale, 1.0f / v_scale, heads, k_scales, v_scales);
  return (int)hipGetLastError();
}

// Observation for the calibration of the FP8 cache (ivg_kv_calibrate): per head, the maximum of |x| over trajectories, rows [0, L) and
// elements of one layer's bf16 K and V ([B * heads][Lmax][64], what rope_kv just wrote), accumulated into amax [2][heads] (k | v) as
// the fp32 bit pattern of that maximum.  The maximum is taken on the INTEGER pattern of |x| (bits & 0x7fff, widened to fp32 by << 16):
// for non-negative floats the integer order is the value order, NaN patterns rank above Inf above every finite value (a non-finite
// K / V is never hidden), and an integer maximum is associative and commutative -- the result does not depend on any order.  That is
// why the atomicMax across workgroups below is within the rule "no atomics on data": the rule is about results that depend on the
// order of arrival, and this one cannot.  One workgroup per (32 rows, b * heads + h) as kv8_pack_kernel, 16-byte loads, rows >= L
// never read, wave reduction by shuffles, one atomic per wave and tensor.
__global__ __launch_bounds__(256) void kv_absmax_kernel(const bf16_t* __restrict__ k16, const bf16_t* __restrict__ v16, int L, int Lmax, int heads,
                                                        unsigned int* __restrict__ amax) {
  const int bh = blockIdx.y, tid = threadIdx.x;
  const int row = blockIdx.x * 32 + (tid >> 3), sub = tid & 7;
  unsigned int mk = 0u, mv = 0u;
  if (row < L) {
    const long off = ((long)bh * Lmax + row) * 64 + sub * 8;
    const Chunk16 a = *(const Chunk16*)(k16 + off), c = *(const Chunk16*)(v16 + off);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      mk = max(mk, max(a[w] & 0x7fffu, (a[w] >> 16) & 0x7fffu));
      mv = max(mv, max(c[w] & 0x7fffu, (c[w] >> 16) & 0x7fffu));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mk = max(mk, (unsigned int)__shfl_xor((int)mk, d, 64));
    mv = max(mv, (unsigned int)__shfl_xor((int)mv, d, 64));
  }
  if ((tid & 63) == 0) {
    const int h = bh % heads;
    if (mk) atomicMax(amax + h, mk << 16);
    if (mv) atomicMax(amax + heads + h, mv << 16);
  }
}

int launch_kv_absmax(const void* k16, const void* v16, int B, int heads, int L, int Lmax, unsigned int* amax, hipStream_t st) {
  if (B <= 0 || heads <= 0 || L < 0 || L > Lmax || !amax) return (int)hipErrorInvalidValue;
  if (L == 0) return 0;
  hipLaunchKernelGGL(kv_absmax_kernel, dim3((unsigned)cdiv(L, 32), (unsigned)(B * heads)), dim3(256), 0, st, (const bf16_t*)k16, (const bf16_t*)v16, L,
                     Lmax, heads, amax);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ sampling
// One workgroup per trajectory.  Restates HF TopKLogitsWarper(top_k) + softmax + one draw as an
// explicit-uniform inverse CDF over the kept tokens in ascending id order (oracle/llama.py
// sample_from_logits); uniforms == null -> greedy argmax (lowest id on ties).  Then embeds the decided
// token as the next input row and (forced sdf slots) adds the action embedding.
__device__ __forceinline__ unsigned f2key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // monotone: larger float -> larger key
}

constexpr int SAMPLE_CAP = 1024;  // kept-token list (ids + values) of the fast inverse-CDF path

// exclusive suffix sum over the 256 threads of a workgroup (thread t receives the sum of threads t+1 .. 255)
__device__ __forceinline__ int block_suffix_excl(int x, int* s4, int lane, int wv) {
  int incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int dn = __shfl_down(incl, o, 64);
    if (lane + o < 64) incl += dn;
  }
  if (lane == 0) s4[wv] = incl;  // wave total
  __syncthreads();
  int above = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) if (w > wv) above += s4[w];
  __syncthreads();
  return incl - x + above;
}

// order key of the nucleus filter: f2key with -0.0 folded onto +0.0, so that key order is exactly the float order l_j <= l_i
__device__ __forceinline__ unsigned nkey(float f) { return f == 0.0f ? 0x80000000u : f2key(f); }

// fp64 sum over the 256 threads of a workgroup in one fixed order (xor butterfly, then waves 0..3): every thread gets the same value
__device__ __forceinline__ double block_sum_f64(double x, double* s_w, int lane, int wv) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if (lane == 0) s_w[wv] = x;
  __syncthreads();
  const double t = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  return t;
}

// NUCLEUS (a.top_p < 1; include/ivg.h ivg_set_top_p): after the top-k filter a kept token i survives iff
// S(i) = sum of e_j = exp(l_j - max) over the kept j with l_j <= l_i exceeds (1 - top_p) * Z, Z the sum over every kept token (fp64),
// or l_i is the maximum.  The instances without it are the sampler as it was: every NUCLEUS branch is `if constexpr`.
template <typename T, int KPT, bool NUCLEUS>  // KPT logits per thread (contiguous segment): vocab <= 256 * KPT
__global__ __launch_bounds__(256) void sample_embed_kernel(SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lg = (float*)smem;  // [V] staging: coalesced global read, then each thread takes a contiguous segment
  __shared__ float s_f[4];
  __shared__ int s_i[4];
  __shared__ int s4[4];
  __shared__ int s_sel[2];
  __shared__ __attribute__((aligned(16))) int hist[2048];
  __shared__ int kid[SAMPLE_CAP];
  __shared__ __attribute__((aligned(16))) float cval[SAMPLE_CAP];
  __shared__ double s_w[4];
  __shared__ long s_tok;
  __shared__ double s_target;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = a.state->j;
  const int V = a.V;
  const bool forced = a.forced_period > 0 && (j % a.forced_period) == 0;
  long tok = 0;
  if (forced) {
    tok = a.forced_token;
  } else if (j == 0) {
    // step 0 only ever FEEDS the prompt's last token (kept-cache and shared-context rollouts: the cache holds positions [0, L0 - 1)):
    // nothing is decided, the token is read back from the id row (the store below rewrites it with itself)
    tok = a.ids_out[(long)b * a.ids_stride + a.L0 - 1];
  } else {
    const float* src = a.logits + (long)b * V;
    if ((V & 1) == 0 && (((uintptr_t)src) & 7) == 0) {
      // 8-byte loads, 16 in flight per lane (one workgroup per trajectory: only B CUs pull the logits, so the row must
      // arrive in as few round trips as possible; a scalar loop here was most of the kernel's time)
      const float2* src2 = (const float2*)src;
      float2* lg2 = (float2*)lg;
      const int n2 = V >> 1;
      for (int i0b = 0; i0b < n2; i0b += 256 * 16) {
        float2 tmp[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { const int i = i0b + r * 256 + tid; tmp[r] = i < n2 ? src2[i] : float2{0.f, 0.f}; }
#pragma unroll
        for (int r = 0; r < 16; ++r) { const int i = i0b + r * 256 + tid; if (i < n2) lg2[i] = tmp[r]; }
      }
    } else {
      for (int i = tid; i < V; i += 256) lg[i] = src[i];
    }
    if (tid == 0) s_tok = -1;
    __syncthreads();
    // HF TemperatureLogitsWarper runs BEFORE the top-k filter: scores = scores / temperature in fp32 (IEEE division, as torch's);
    // every later read of the row (candidates, exponentials) sees the scaled values.  1.0 (every caller of the reference): untouched.
    if (a.temperature != 1.0f) {
      for (int i = tid; i < V; i += 256) lg[i] = lg[i] / a.temperature;
      __syncthreads();
    }
    const int seg = (V + 255) / 256;
    const int i0 = tid * seg;
    const int nvalid = max(0, min(seg, V - i0));   // this thread owns ids [i0, i0 + nvalid)
    float v[KPT];
    float mx = -INFINITY;
    int mi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < KPT; ++q) v[q] = lg[min(i0 + q, V - 1)];   // unconditional: all reads are issued back to back
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      if (q >= nvalid) v[q] = -INFINITY;
      if (v[q] > mx) { mx = v[q]; mi = i0 + q; }  // ascending index: the first maximum is kept
    }
    const float tmax = mx;   // this thread's own maximum (pivot pre-filter of the sampler below)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // (max, lowest index) reduction
      const float ov = __shfl_xor(mx, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
    }
    if (lane == 0) { s_f[wv] = mx; s_i[wv] = mi; }
    __syncthreads();
    mx = s_f[0]; mi = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) if (s_f[w] > mx || (s_f[w] == mx && s_i[w] < mi)) { mx = s_f[w]; mi = s_i[w]; }
    if (a.uniforms == nullptr) {
      tok = mi;
    } else {
      // ---- key of the k-th largest logit (= largest T with #{key >= T} >= k).  General method: radix select, digits of
      //      11 / 11 / 10 bits, one LDS histogram per digit over the keys that match the digits found so far (exact counts)
      unsigned key[KPT];   // filled by the radix path only
      int kk = a.top_k < V ? a.top_k : V;
      unsigned thr = 0u;
      bool have_thr = false;
      int n_list = -1;                              // >= 0: (key, id, value) lists in LDS, ascending id order
      unsigned* s_ck = (unsigned*)hist + 256;       // [SAMPLE_CAP] keys of the listed tokens (hist is free when they are written)
      if (kk <= 256) {
        // Pre-filter (k <= 256): in every wave take the ceil(k/4)-th largest of its 64 per-thread maxima; the smallest of the
        // four is a lower bound of the k-th largest logit (at least k distinct elements are >= it), so only the tokens >=
        // that pivot -- a few more than k of them -- can hold the threshold.  They are listed once (key, id, value;
        // ascending id) and ranked against each other by counting: no histogram atomics and no second sweep over the
        // vocabulary on the hot path.
        const unsigned mine = f2key(tmax);
        int rank = 0;
#pragma unroll
        for (int jl = 0; jl < 64; ++jl) {
          const unsigned o = (unsigned)__builtin_amdgcn_readlane((int)mine, jl);
          rank += (o > mine || (o == mine && jl < lane)) ? 1 : 0;
        }
        if (rank == (kk + 3) / 4 - 1) s4[wv] = (int)mine;   // ranks are a permutation of 0..63: one writer per wave
        __syncthreads();
        unsigned pivot = (unsigned)s4[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) pivot = (unsigned)s4[w] < pivot ? (unsigned)s4[w] : pivot;
        const float pivf = __uint_as_float((pivot & 0x80000000u) ? (pivot & 0x7fffffffu) : ~pivot);   // inverse of f2key
        unsigned cm[(KPT + 31) / 32];
#pragma unroll
        for (int w = 0; w < (KPT + 31) / 32; ++w) cm[w] = 0u;
#pragma unroll
        for (int q = 0; q < KPT; ++q) cm[q >> 5] |= (q < nvalid && v[q] >= pivf) ? (1u << (q & 31)) : 0u;
        int cc = 0;
#pragma unroll
        for (int w = 0; w < (KPT + 31) / 32; ++w) cc += __builtin_popcount(cm[w]);
        __syncthreads();                             // every thread has read s4
        const int hi = block_suffix_excl(cc, s4, lane, wv);
        if (tid == 0) s_sel[1] = hi + cc;           // number of candidates (>= k)
        __syncthreads();
        const int n_c = s_sel[1];
        if (n_c <= SAMPLE_CAP) {
          int off = n_c - hi - cc;                   // candidates in lower threads = lower ids
#pragma unroll
          for (int w = 0; w < (KPT + 31) / 32; ++w) {
            unsigned mm = cm[w];
            while (mm) {                             // a thread holds 0-3 candidates: read them back from the staged row
              const int id = i0 + w * 32 + __builtin_ctz(mm);
              mm &= mm - 1;
              const float val = lg[id];
              s_ck[off] = f2key(val); kid[off] = id; cval[off] = val; ++off;
            }
          }
          if (tid < 4) s_ck[n_c + tid] = 0u;           // pad to a multiple of 4 (hist has room beyond CAP)
          __syncthreads();
          unsigned best = 0xffffffffu;               // smallest candidate with fewer than k strictly larger ones = k-th largest
          const uint4* c4 = (const uint4*)s_ck;
          const int n4 = (n_c + 3) >> 2;
          for (int i = tid; i < n_c; i += 256) {
            const unsigned ci = s_ck[i];
            int g = 0;
#pragma unroll 8
            for (int j4 = 0; j4 < n4; ++j4) {
              const uint4 o = c4[j4];
              g += (o.x > ci ? 1 : 0) + (o.y > ci ? 1 : 0) + (o.z > ci ? 1 : 0) + (o.w > ci ? 1 : 0);
            }
            if (g < kk && ci < best) best = ci;
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) { const unsigned ob = __shfl_xor(best, o, 64); best = ob < best ? ob : best; }
          if (lane == 0) s4[wv] = (int)best;
          __syncthreads();
          thr = (unsigned)s4[0];
#pragma unroll
          for (int w = 1; w < 4; ++w) thr = (unsigned)s4[w] < thr ? (unsigned)s4[w] : thr;
          have_thr = true;
          n_list = n_c;
          __syncthreads();                           // s4 is reused below
        }
      }
      if (!have_thr) {   // k > 256 or a flood of candidates (massive ties): radix select over all keys
#pragma unroll
      for (int q = 0; q < KPT; ++q) key[q] = f2key(v[q]);
      unsigned prefix = 0u, pmask = 0u;
#pragma unroll
      for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const int nb = pass == 2 ? 1024 : 2048, per = nb / 256;
        for (int i = tid; i < nb; i += 256) hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KPT; ++q)
          if (q < seg && i0 + q < V && (key[q] & pmask) == prefix) atomicAdd(&hist[(key[q] >> shift) & (nb - 1)], 1);
        __syncthreads();
        int mine = 0;
        for (int r = 0; r < per; ++r) mine += hist[tid * per + r];
        const int above = block_suffix_excl(mine, s4, lane, wv);  // keys in bins above this thread's bins
        if (above < kk && kk <= above + mine) {                    // exactly one thread: the digit is in its bins
          int acc = above, d = tid * per + per - 1;
          for (; d > tid * per; --d) { if (acc + hist[d] >= kk) break; acc += hist[d]; }
          s_sel[0] = d; s_sel[1] = kk - acc;
        }
        __syncthreads();
        prefix |= (unsigned)s_sel[0] << shift;
        pmask |= (unsigned)(nb - 1) << shift;
        kk = s_sel[1];
      }
      thr = prefix;
      }
      // everything >= thr is kept (ties at the threshold included, as HF's masked_fill)
      // ---- inverse CDF in ascending id order, fp64 (oracle: double cumsum of exp(logit - max) over the kept ids)
      if (n_list < 0) {   // radix path: list the kept tokens now
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < KPT; ++q) cnt += (key[q] >= thr && v[q] > -INFINITY) ? 1 : 0;
        const int after = block_suffix_excl(cnt, s4, lane, wv);
        if (tid == 0) s_sel[0] = after + cnt;  // number of kept tokens
        __syncthreads();
        const int n_kept = s_sel[0];
        if (n_kept <= SAMPLE_CAP) {
          int off = n_kept - after - cnt;  // kept tokens in lower threads = lower ids
#pragma unroll
          for (int q = 0; q < KPT; ++q)
            if (key[q] >= thr && v[q] > -INFINITY) { s_ck[off] = key[q]; cval[off] = v[q]; kid[off] = i0 + q; ++off; }
          __syncthreads();
          n_list = n_kept;
        }
      }
      if (n_list >= 0) {
        // the listed tokens (about top_k of them) are spread over the threads, so the fp64 exponentials run once each, in
        // parallel; listed tokens below the threshold (pre-filter path) weigh zero, exactly as in the oracle's masked sum
        const int per = (n_list + 255) / 256;  // <= 4
        const int e0 = tid * per, e1 = min(n_list, e0 + per);
        double ex[SAMPLE_CAP / 256];
        double part = 0.0;
#pragma unroll
        for (int r = 0; r < SAMPLE_CAP / 256; ++r) {
          ex[r] = 0.0;
          if (r < per) {   // uniform across the workgroup
            if (e0 + r < e1 && s_ck[e0 + r] >= thr && cval[e0 + r] > -INFINITY) ex[r] = exp((double)(cval[e0 + r] - mx));
            part += ex[r];
          }
        }
        if constexpr (NUCLEUS) {
          // S(i) by counting over the list: each listed token sums the weights of the listed tokens not above it (ascending
          // id order, fp64).  The weights go to the staging row, free once the list is built (the launch gives it >= 8 KiB).
          double* s_e = (double*)lg;
#pragma unroll
          for (int r = 0; r < SAMPLE_CAP / 256; ++r)
            if (r < per && e0 + r < e1) s_e[e0 + r] = ex[r];
          if (tid < 8 && n_list + tid < SAMPLE_CAP) s_e[n_list + tid] = 0.0;   // pad to a multiple of 8: weightless
          const double cut = (1.0 - (double)a.top_p) * block_sum_f64(part, s_w, lane, wv);   // (synchronises: s_e is complete)
          part = 0.0;
#pragma unroll
          for (int r = 0; r < SAMPLE_CAP / 256; ++r) {
            if (r < per && ex[r] > 0.0) {
              // the list padded to a multiple of 8 with weightless entries, read 16 bytes at a time, 8 independent fp64 chains combined
              // in one fixed order: a single chain over ~150 entries waited on LDS and add latency at every step (+10 us per launch)
              const float li = cval[e0 + r];
              double S = 0.0;
              const int n8 = (n_list + 7) & ~7;
              double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0, S5 = 0.0, S6 = 0.0, S7 = 0.0;
#pragma unroll 2
              for (int jj = 0; jj < n8; jj += 8) {
                const float4 ca = *(const float4*)&cval[jj], cb = *(const float4*)&cval[jj + 4];
                const double2 ea = *(const double2*)&s_e[jj], eb = *(const double2*)&s_e[jj + 2];
                const double2 ec = *(const double2*)&s_e[jj + 4], ed = *(const double2*)&s_e[jj + 6];
                S0 += ca.x <= li ? ea.x : 0.0; S1 += ca.y <= li ? ea.y : 0.0; S2 += ca.z <= li ? eb.x : 0.0; S3 += ca.w <= li ? eb.y : 0.0;
                S4 += cb.x <= li ? ec.x : 0.0; S5 += cb.y <= li ? ec.y : 0.0; S6 += cb.z <= li ? ed.x : 0.0; S7 += cb.w <= li ? ed.y : 0.0;
              }
              S = ((S0 + S1) + (S2 + S3)) + ((S4 + S5) + (S6 + S7));
              if (!(S > cut || li == mx)) ex[r] = 0.0;
            }
            part += ex[r];
          }
        }
        double incl = part;  // inclusive scan over threads (thread order == id order)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const double up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        double base = 0.0, total = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wv) base += s_w[w]; total += s_w[w]; }
        incl += base;
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = base;
        const double target = (double)a.uniforms[(long)b * a.n_uni + (j - 1)] * total;
        // intervals [excl, incl) tile [0, total) exactly (incl of thread t IS excl of thread t+1)
        if (part > 0.0 && excl <= target && target < incl) {
          double run = excl;
          int found = -1, last = -1;
#pragma unroll
          for (int r = 0; r < SAMPLE_CAP / 256; ++r)
            if (r < per && ex[r] > 0.0) { run += ex[r]; last = kid[e0 + r]; if (found < 0 && run > target) found = last; }
          s_tok = found >= 0 ? found : last;  // rounding at the chunk edge: the chunk's last kept token
        }
        __syncthreads();
        tok = s_tok;
        if (tok < 0) tok = mi;  // unreachable for u in [0, 1): defensive
      } else {
        // general path (massive ties at the threshold): every thread walks its own id segment
        unsigned tau = 0u;   // NUCLEUS: the survivors are the kept tokens with nkey >= tau
        if constexpr (NUCLEUS) {
          // tau = the smallest key T with G(T) = sum of the kept weights with nkey <= T above the cut (G is monotone in T):
          // 32 rounds of bisection over the key space, each one fixed-order fp64 block sum (deterministic, no atomics)
          double e[KPT];
          double zp = 0.0;
#pragma unroll
          for (int q = 0; q < KPT; ++q) {
            e[q] = (key[q] >= thr && v[q] > -INFINITY) ? exp((double)(v[q] - mx)) : 0.0;
            zp += e[q];
          }
          const double Z = block_sum_f64(zp, s_w, lane, wv);
          const double cut = (1.0 - (double)a.top_p) * Z;
          unsigned lo = 0u, hi = 0xffffffffu;
          if (!(Z > cut)) lo = hi;   // top_p = 0 (or nothing kept): the maximum alone
          while (lo < hi) {          // uniform: every thread holds the same sums
            const unsigned mid = lo + ((hi - lo) >> 1);
            double m = 0.0;
#pragma unroll
            for (int q = 0; q < KPT; ++q) m += nkey(v[q]) <= mid ? e[q] : 0.0;
            if (block_sum_f64(m, s_w, lane, wv) > cut) hi = mid; else lo = mid + 1;
          }
          tau = min(lo, nkey(mx));   // the maximum always survives
        }
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < KPT; ++q)
          if (key[q] >= thr && v[q] > -INFINITY && (!NUCLEUS || nkey(v[q]) >= tau)) part += exp((double)(v[q] - mx));
        double incl = part;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const double up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        double base = 0.0, total = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wv) base += s_w[w]; total += s_w[w]; }
        incl += base;
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = base;
        if (tid == 0) s_target = (double)a.uniforms[(long)b * a.n_uni + (j - 1)] * total;
        __syncthreads();
        const double target = s_target;
        if (part > 0.0 && excl <= target && target < incl) {
          double run = excl;
          long found = -1, last = -1;
#pragma unroll
          for (int q = 0; q < KPT; ++q) {
            if (key[q] >= thr && v[q] > -INFINITY && (!NUCLEUS || nkey(v[q]) >= tau)) {
              run += exp((double)(v[q] - mx));
              last = i0 + q;
              if (found < 0 && run > target) found = i0 + q;
            }
          }
          s_tok = found >= 0 ? found : last;
        }
        __syncthreads();
        tok = s_tok;
        if (tok < 0) tok = mi;
      }
    }
  }
  // a row of NaN / -inf logits leaves the arg-max index at its initial value: never let it reach the id buffer or the
  // embedding gather (out-of-bounds read inside a replayed graph); such a row decides token 0
  if (tok < 0 || tok >= V) tok = 0;
  if (tid == 0) a.ids_out[(long)b * a.ids_stride + a.L0 + (j - 1)] = (int64_t)tok;
  // ---- next input embedding
  const T* src = (const T*)a.E + tok * a.H;
  T* dst = (T*)a.x + (long)b * a.H;
  const T* act = nullptr;
  if (forced && a.act) act = (const T*)a.act + ((long)b * a.act_T + (a.slot0 + j / a.forced_period + a.ctx - 1)) * a.H;
  for (int c = tid; c < a.H; c += 256) {
    float val = to_f32(src[c]);
    if (act) val += to_f32(act[c]);
    dst[c] = from_f32<T>(val);
  }
}

template <typename T, int KPT, bool NUCLEUS>
static void launch_sample_t(const SampleArgs& a, int B, size_t smem, hipStream_t st) {
  static DynLdsOnce once;
  (void)ensure_dyn_lds(once, (const void*)sample_embed_kernel<T, KPT, NUCLEUS>, 96 * 1024);
  hipLaunchKernelGGL((sample_embed_kernel<T, KPT, NUCLEUS>), dim3(B), dim3(256), smem, st, a);
}

template <bool NUCLEUS>
static void launch_sample_dt(const SampleArgs& a, int B, DType dt, size_t smem, hipStream_t st) {
  const bool small = a.V <= 256 * 36;
  if (dt == BF16) { if (small) launch_sample_t<bf16_t, 36, NUCLEUS>(a, B, smem, st); else launch_sample_t<bf16_t, 72, NUCLEUS>(a, B, smem, st); }
  else { if (small) launch_sample_t<float, 36, NUCLEUS>(a, B, smem, st); else launch_sample_t<float, 72, NUCLEUS>(a, B, smem, st); }
}

int launch_sample_embed(const SampleArgs& a, int B, DType dt, hipStream_t st) {
  const size_t smem = (size_t)std::max(a.V, SAMPLE_CAP) * sizeof(float);
  if (a.V > 256 * 72 || smem > 96 * 1024) return (int)hipErrorInvalidValue;
  if (a.top_p < 1.0f)   // the nucleus filter keeps the list's fp64 weights in the staging row: SAMPLE_CAP doubles
    launch_sample_dt<true>(a, B, dt, std::max(smem, (size_t)SAMPLE_CAP * sizeof(double)), st);
  else
    launch_sample_dt<false>(a, B, dt, smem, st);
  return (int)hipGetLastError();
}

__global__ void state_set_kernel(StepState* s, int pos, int j) { s->pos = pos; s->j = j; }

int launch_state_set(StepState* state, int pos, int j, hipStream_t st) {
  hipLaunchKernelGGL(state_set_kernel, dim3(1), dim3(1), 0, st, state, pos, j);
  return (int)hipGetLastError();
}

// ids[r][0 .. L) = prompts[(b0 + r) / G][0 .. L): every trajectory of a group starts from a copy of its group's prompt
__global__ void expand_prompt_rows_kernel(const int64_t* __restrict__ prompts, long pstride, int64_t* __restrict__ ids, long ids_ld, int L,
                                          int G, int b0) {
  const int r = blockIdx.y;
  const int64_t* src = prompts + (long)((b0 + r) / G) * pstride;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < L; c += gridDim.x * blockDim.x) ids[(long)r * ids_ld + c] = src[c];
}

int launch_expand_prompt_rows(const int64_t* prompts, long pstride, int64_t* ids, long ids_ld, int rows, int L, int G, int b0, hipStream_t st) {
  if (rows <= 0 || L <= 0) return 0;
  hipLaunchKernelGGL(expand_prompt_rows_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)rows), dim3(256), 0, st, prompts, pstride, ids, ids_ld, L, G, b0);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ small heads
template <typename T>
__global__ __launch_bounds__(256) void action_embed_kernel(const float* __restrict__ act, const float* __restrict__ W,
                                                           const float* __restrict__ bias, T* __restrict__ out, int A, int H) {
  const int row = blockIdx.x;
  for (int c = threadIdx.x; c < H; c += 256) {
    float s = 0.f;
    for (int k = 0; k < A; ++k) s = fmaf(act[(long)row * A + k], W[(long)c * A + k], s);
    out[(long)row * H + c] = from_f32<T>(s + bias[c]);
  }
}

int launch_action_embed(const float* act, const float* W, const float* bias, void* out, DType dt, int BT, int A, int H,
                        hipStream_t st) {
  if (BT <= 0) return 0;
  if (dt == BF16) hipLaunchKernelGGL(action_embed_kernel<bf16_t>, dim3(BT), dim3(256), 0, st, act, W, bias, (bf16_t*)out, A, H);
  else hipLaunchKernelGGL(action_embed_kernel<float>, dim3(BT), dim3(256), 0, st, act, W, bias, (float*)out, A, H);
  return (int)hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(256) void add_rows_kernel(T* __restrict__ x, long xs, const T* __restrict__ add, long as, int H) {
  const int b = blockIdx.x;
  for (int c = threadIdx.x; c < H; c += 256) x[b * xs + c] = from_f32<T>(to_f32(x[b * xs + c]) + to_f32(add[b * as + c]));
}

int launch_add_rows(void* x, long x_stride, const void* add, long add_stride, int B, int H, DType dt, hipStream_t st) {
  if (B <= 0) return 0;
  if (dt == BF16) hipLaunchKernelGGL(add_rows_kernel<bf16_t>, dim3(B), dim3(256), 0, st, (bf16_t*)x, x_stride, (const bf16_t*)add, add_stride, H);
  else hipLaunchKernelGGL(add_rows_kernel<float>, dim3(B), dim3(256), 0, st, (float*)x, x_stride, (const float*)add, add_stride, H);
  return (int)hipGetLastError();
}

// r[b] = rsqrt(mean(h^2) + eps) * dot(h[b], w) + bias: reward head on the final-normed hidden state (norm weight folded into w)
template <typename T>
__global__ __launch_bounds__(64) void rowdot_kernel(const T* __restrict__ h, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ out, int H, float eps) {
  const int b = blockIdx.x;
  float s = 0.f, ss = 0.f;
  for (int c = threadIdx.x; c < H; c += 64) { const float v = to_f32(h[(long)b * H + c]); s = fmaf(v, w[c], s); ss = fmaf(v, v, ss); }
  s = wave_sum(s);
  ss = wave_sum(ss);
  if (threadIdx.x == 0) out[b] = (eps >= 0.f ? s * rsqrtf(ss / (float)H + eps) : s) + bias[0];   // eps < 0: h is already normed
}

int launch_rowdot(const void* h, const float* w, const float* bias, float* out, int B, int H, float eps, DType dt, hipStream_t st) {
  if (B <= 0) return 0;
  if (dt == BF16) hipLaunchKernelGGL(rowdot_kernel<bf16_t>, dim3(B), dim3(64), 0, st, (const bf16_t*)h, w, bias, out, H, eps);
  else hipLaunchKernelGGL(rowdot_kernel<float>, dim3(B), dim3(64), 0, st, (const float*)h, w, bias, out, H, eps);
  return (int)hipGetLastError();
}

// out[b][:] = w * T(x[b][:] * rsqrt(mean x^2 + eps))  -- HF LlamaRMSNorm: the normalised row is rounded to the model dtype before
// the weight multiplies it.  This is `hidden_states[-1]` of the last layer as HF reports it (post final norm).
template <typename T>
__global__ __launch_bounds__(256) void final_hidden_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ out,
                                                           int H, float eps) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  float ss = 0.f;
  for (int c = tid; c < H; c += 256) { const float v = to_f32(x[(long)b * H + c]); ss = fmaf(v, v, ss); }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float rs = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + eps);
  for (int c = tid; c < H; c += 256) {
    const T n = from_f32<T>(to_f32(x[(long)b * H + c]) * rs);
    out[(long)b * H + c] = from_f32<T>(to_f32(from_f32<T>(w[c])) * to_f32(n));
  }
}

int launch_final_hidden(const void* x, const float* w, void* out, int B, int H, float eps, DType dt, hipStream_t st) {
  if (B <= 0) return 0;
  if (dt == BF16) hipLaunchKernelGGL(final_hidden_kernel<bf16_t>, dim3(B), dim3(256), 0, st, (const bf16_t*)x, w, (bf16_t*)out, H, eps);
  else hipLaunchKernelGGL(final_hidden_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)x, w, (float*)out, H, eps);
  return (int)hipGetLastError();
}

// Per-frame heads of a forced-sdf rollout (include/ivg.h ivg_generate_frames), one launch per decode step between the last
// down-projection and lm_head (which advances the state): state->j is the new token this step FED.  Nothing happens unless that token
// is a frame's 16th, j = 17 i + 16; then workgroup b leaves frame i of trajectory b: hid[b][i][:] with final_hidden_kernel's
// arithmetic (all four waves) and rew[b][i] with rowdot_kernel's (wave 0 alone, its own stride-64 sums), so that either equals what
// those kernels give on the same row bit for bit.  F: frames a row of rew / hid holds; a frame beyond it is never written.
// One residual row through both heads, by a workgroup of 256 threads (red: 4 floats of LDS): hid_out[:] with final_hidden_kernel's
// arithmetic (all four waves), *rew_out with rowdot_kernel's (wave 0 alone, its own stride-64 sums); either may be null
template <typename T>
__device__ __forceinline__ void frame_heads_row(const T* __restrict__ row, const float* __restrict__ rew_w, const float* __restrict__ rew_b,
                                                const float* __restrict__ norm_w, float* __restrict__ rew_out, T* __restrict__ hid_out, int H,
                                                float eps, float* red) {
  const int tid = threadIdx.x;
  if (hid_out) {
    float ss = 0.f;
    for (int c = tid; c < H; c += 256) { const float v = to_f32(row[c]); ss = fmaf(v, v, ss); }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float rs = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + eps);
    for (int c = tid; c < H; c += 256) {
      const T n = from_f32<T>(to_f32(row[c]) * rs);
      hid_out[c] = from_f32<T>(to_f32(from_f32<T>(norm_w[c])) * to_f32(n));
    }
  }
  if (rew_out && tid < 64) {
    float s = 0.f, ss = 0.f;
    for (int c = tid; c < H; c += 64) { const float v = to_f32(row[c]); s = fmaf(v, rew_w[c], s); ss = fmaf(v, v, ss); }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (tid == 0) {
      // rowdot_kernel rounds the product before it adds the bias (its select keeps the two apart): no contraction into an fma here
#pragma clang fp contract(off)
      const float r = s * rsqrtf(ss / (float)H + eps);
      *rew_out = r + rew_b[0];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void frame_heads_kernel(const T* __restrict__ x, const StepState* __restrict__ state, const float* __restrict__ rew_w,
                                                          const float* __restrict__ rew_b, const float* __restrict__ norm_w,
                                                          float* __restrict__ rew, T* __restrict__ hid, int H, int F, float eps) {
  const int j = state->j;
  if (j % 17 != 16) return;
  const int i = j / 17;
  if (i >= F) return;
  __shared__ float red[4];
  const int b = blockIdx.x;
  frame_heads_row<T>(x + (long)b * H, rew_w, rew_b, norm_w, rew ? rew + (long)b * F + i : nullptr, hid ? hid + ((long)b * F + i) * H : nullptr, H, eps, red);
}

int launch_frame_heads(const void* x, const StepState* state, const float* rew_w, const float* rew_b, const float* norm_w, float* rew, void* hid,
                       int B, int H, int F, float eps, DType dt, hipStream_t st) {
  if (B <= 0 || F <= 0 || (!rew && !hid)) return 0;
  if ((rew && !(rew_w && rew_b)) || (hid && !norm_w)) return (int)hipErrorInvalidValue;
  if (dt == BF16) hipLaunchKernelGGL(frame_heads_kernel<bf16_t>, dim3(B), dim3(256), 0, st, (const bf16_t*)x, state, rew_w, rew_b, norm_w, rew, (bf16_t*)hid, H, F, eps);
  else hipLaunchKernelGGL(frame_heads_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)x, state, rew_w, rew_b, norm_w, rew, (float*)hid, H, F, eps);
  return (int)hipGetLastError();
}

// The same heads on residual rows picked out of a matrix of rows (ivg_kv_extend_scored): workgroup (b, k) = (blockIdx.x / F, blockIdx.x % F)
// reads row row0 + b * row_stride + k * frame_stride of x and writes rew[b * out_F + out_k0 + k] and hid[b * out_F + out_k0 + k][:] -- the
// caller's own buffers.  The chunk pass: rows b * T + (q_i - keep_len) of its residual stream, all frames in one launch (frame_stride 17);
// a decode step that fed a frame's 16th token: the B rows of the step buffer, F = 1, out_k0 the frame's column.
template <typename T>
__global__ __launch_bounds__(256) void frame_rows_heads_kernel(const T* __restrict__ x, long row0, long row_stride, long frame_stride,
                                                               const float* __restrict__ rew_w, const float* __restrict__ rew_b,
                                                               const float* __restrict__ norm_w, float* __restrict__ rew, T* __restrict__ hid,
                                                               int H, int F, int out_k0, int out_F, float eps) {
  __shared__ float red[4];
  const long b = blockIdx.x / F, k = blockIdx.x - b * F;
  const long o = b * out_F + out_k0 + k;
  frame_heads_row<T>(x + (row0 + b * row_stride + k * frame_stride) * H, rew_w, rew_b, norm_w, rew ? rew + o : nullptr, hid ? hid + o * H : nullptr, H,
                     eps, red);
}

int launch_frame_rows_heads(const void* x, long row0, long row_stride, long frame_stride, const float* rew_w, const float* rew_b, const float* norm_w,
                            float* rew, void* hid, int B, int H, int F, int out_k0, int out_F, float eps, DType dt, hipStream_t st) {
  if (B <= 0 || F <= 0 || (!rew && !hid)) return 0;
  if ((rew && !(rew_w && rew_b)) || (hid && !norm_w) || out_k0 < 0 || out_k0 + F > out_F) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)B * (unsigned)F);
  if (dt == BF16)
    hipLaunchKernelGGL(frame_rows_heads_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, row0, row_stride, frame_stride, rew_w, rew_b, norm_w, rew,
                       (bf16_t*)hid, H, F, out_k0, out_F, eps);
  else
    hipLaunchKernelGGL(frame_rows_heads_kernel<float>, grid, dim3(256), 0, st, (const float*)x, row0, row_stride, frame_stride, rew_w, rew_b, norm_w, rew,
                       (float*)hid, H, F, out_k0, out_F, eps);
  return (int)hipGetLastError();
}

static std::atomic<long long> g_frame_heads_hits{0};
void frame_heads_note(int hits) { g_frame_heads_hits += hits; }
long long frame_heads_hits() { return g_frame_heads_hits.load(); }

// Token scores of a rollout (include/ivg.h ivg_generate_scored), one launch per decode step directly after the sampler: state->j is
// the new token the sampler just DECIDED, ids[b][L0 + j - 1] the id it stored, logits[b][:] the raw fp32 row it read (before the
// temperature division and the top-k / top-p filters; lm_head of this step overwrites it later in stream order).  Workgroup b leaves
// out[b][j - 1][0..2] = { z[tok] - lse(z), H(softmax(z)), max(z) - lse(z) }; a forced column (j % period == 0) gets three zeros,
// j = 0 (the step that only feeds the prompt's last token) and j > cols write nothing.  fp32, max subtraction, entropy as
// log s - (sum e_i (z_i - m)) / s with the terms of e_i == 0 left out (rows may hold -inf); a maximum that is not finite gives NaN
// in all three, an id outside [0, V) a NaN logprob without a read.  Element i belongs to thread (i / 4) % 256 whatever the row's
// alignment (16-, 8- or 4-byte loads), and the sums run in one fixed order (thread, wave butterfly, waves 0..3): no atomics, the same
// bits on every run, in a replayed graph and for a row at any place in the batch.  The sampler's own instances are untouched.
constexpr int SCORE_GROUPS = 18;   // 4 logits each: vocab <= 256 * 72, the sampler's own limit
// The three scores of one logits row against the id `tok`, by a workgroup of 256 threads (red: 12 floats of LDS); thread 0 writes o[0..2]
__device__ __forceinline__ void token_scores_row(const float* __restrict__ row, int V, long tok, float* __restrict__ o, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int al = (int)(((uintptr_t)row) & 15);
  float v[4 * SCORE_GROUPS];
#pragma unroll
  for (int q = 0; q < SCORE_GROUPS; ++q) {
    const int i = (q * 256 + tid) * 4;
    float4 t = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // past the row: weight 0 in every sum
    if (i + 3 < V) {
      if (al == 0) t = *(const float4*)(row + i);
      else if ((al & 7) == 0) { const float2 a = *(const float2*)(row + i), c = *(const float2*)(row + i + 2); t = float4{a.x, a.y, c.x, c.y}; }
      else t = float4{row[i], row[i + 1], row[i + 2], row[i + 3]};
    } else if (i < V) {
      t.x = row[i];
      if (i + 1 < V) t.y = row[i + 1];
      if (i + 2 < V) t.z = row[i + 2];
    }
    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < 4 * SCORE_GROUPS; ++q) mx = fmaxf(mx, v[q]);
  mx = wave_max(mx);
  if (lane == 0) red[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float s = 0.f, t = 0.f;
#pragma unroll
  for (int q = 0; q < 4 * SCORE_GROUPS; ++q) {
    const float d = v[q] - mx, e = expf(d);
    s += e;
    if (e != 0.f) t = fmaf(e, d, t);
  }
  s = wave_sum(s);
  t = wave_sum(t);
  if (lane == 0) { red[4 + wv] = s; red[8 + wv] = t; }
  __syncthreads();
  if (tid == 0) {
    s = (red[4] + red[5]) + (red[6] + red[7]);
    t = (red[8] + red[9]) + (red[10] + red[11]);
    const float ls = logf(s), nan = __int_as_float(0x7fc00000);
    const bool ok = mx > -INFINITY && mx < INFINITY;   // (a NaN among finite entries reaches s and t by itself)
    o[0] = ok && tok >= 0 && tok < V ? (row[tok] - mx) - ls : nan;
    o[1] = ok ? ls - t / s : nan;
    o[2] = ok ? (mx - mx) - ls : nan;   // (the very expression of o[0] at the arg-max: greedy gives the same bits)
  }
}

__global__ __launch_bounds__(256) void token_scores_kernel(const float* __restrict__ logits, int V, const StepState* __restrict__ state,
                                                           const int64_t* __restrict__ ids, long ids_stride, int L0, int forced_period,
                                                           float* __restrict__ out, int cols) {
  const int j = state->j;
  if (j < 1 || j > cols) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  float* o = out + ((long)b * cols + (j - 1)) * 3;
  if (forced_period > 0 && j % forced_period == 0) {
    if (tid < 3) o[tid] = 0.f;
    return;
  }
  __shared__ float red[12];
  token_scores_row(logits + (long)b * V, V, ids[(long)b * ids_stride + L0 + (j - 1)], o, red);
}

int launch_token_scores(const float* logits, int V, const StepState* state, const int64_t* ids, long ids_stride, int L0, int forced_period,
                        float* out, int cols, int B, hipStream_t st) {
  if (B <= 0 || cols <= 0) return 0;
  if (!logits || !ids || !out || V < 1 || V > 256 * 4 * SCORE_GROUPS) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(token_scores_kernel, dim3(B), dim3(256), 0, st, logits, V, state, ids, ids_stride, L0, forced_period, out, cols);
  return (int)hipGetLastError();
}

// The same scores per row of a chunk of teacher-forced logits rows whose targets are given ids (ivg_kv_extend_scored): chunk row i is row
// r = row0 + i of [B][Tc] rows, (b, c) = (r / Tc, r % Tc), as token_nll_kernel; its target is ids[b][c] and its scores go to
// out[(b * out_ld + c) * 3 ..].  Column c is forced (three zeros, the row is not read) when period > 0, c >= first_forced and
// (c - first_forced) % period == 0.
__global__ __launch_bounds__(256) void token_scores_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ ids, long ids_stride,
                                                                long row0, int Tc, int V, int first_forced, int period,
                                                                float* __restrict__ out, long out_ld) {
  const long r = row0 + blockIdx.x;
  const long b = r / Tc, c = r - b * Tc;
  float* o = out + (b * out_ld + c) * 3;
  if (period > 0 && c >= first_forced && (c - first_forced) % period == 0) {
    if (threadIdx.x < 3) o[threadIdx.x] = 0.f;
    return;
  }
  __shared__ float red[12];
  token_scores_row(logits + (long)blockIdx.x * V, V, ids[b * ids_stride + c], o, red);
}

int launch_token_scores_rows(const float* logits, const int64_t* ids, long ids_stride, long row0, int rows, int Tc, int V, int first_forced, int period,
                             float* out, long out_ld, hipStream_t st) {
  if (rows <= 0) return 0;
  if (!logits || !ids || !out || Tc < 1 || row0 < 0 || V < 1 || V > 256 * 4 * SCORE_GROUPS || first_forced < 0 || period < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(token_scores_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, logits, ids, ids_stride, row0, Tc, V, first_forced, period, out,
                     out_ld);
  return (int)hipGetLastError();
}

static std::atomic<long long> g_token_scores_launches{0};
void token_scores_note(int launches) { g_token_scores_launches += launches; }
long long token_scores_launches() { return g_token_scores_launches.load(); }

// Filtered scores of a rollout (include/ivg.h ivg_generate_filtered): the probability of the sampled token under the distribution it was
// DRAWN from -- the row after temperature, top-k and top-p -- one launch per decode step in token_scores_kernel's slot (after the sampler
// stored its id, before this step's lm_head overwrites the row).  A kernel of its own that restates the sampler's filter (ivg_set_top_p
// steps 1-3) in the arithmetic of the sampler's general path; the sampler's instances are untouched.  Element i of the row belongs to
// thread i % 256 (register slot i / 256), every sum is fp64 in one fixed order (slots ascending, wave butterfly, waves 0..3): no atomics,
// the same bits on every run, eager or replayed, for a row at any place in the batch.
__device__ __forceinline__ int block_sum_i32(int x, int* s_c, int lane, int wv) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if (lane == 0) s_c[wv] = x;
  __syncthreads();
  const int t = s_c[0] + s_c[1] + s_c[2] + s_c[3];
  __syncthreads();
  return t;
}

// The four scores of one logits row against the id `tok`, by a workgroup of 256 threads; thread 0 writes o[0..3] = { filtered logprob,
// filtered entropy, kept log-mass, support }.  greedy: no warpers (HF builds none): S is every finite entry of the raw row.
template <int KPT>  // KPT logits per thread: V <= 256 * KPT
__device__ __forceinline__ void filtered_scores_row(const float* __restrict__ row, int V, long tok, int top_k, float temperature, float top_p,
                                                    bool greedy, float* __restrict__ o, double* s_w, int* s_c, float* s_f) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool scale = !greedy && temperature != 1.0f;
  auto key2f = [](unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); };   // inverse of f2key
  unsigned key[KPT];   // f2key of the tempered entry; 0 past the row (below every entry: never counted, never kept)
  float mx = -INFINITY;
  int nans = 0;
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const int i = q * 256 + tid;
    key[q] = 0u;
    if (i < V) {
      float l = row[i];
      if (scale) l = l / temperature;
      key[q] = f2key(l);
      mx = fmaxf(mx, l);
      nans += l != l ? 1 : 0;
    }
  }
  mx = wave_max(mx);
  if (lane == 0) s_f[wv] = mx;
  nans = block_sum_i32(nans, s_c, lane, wv);   // (synchronises: s_f is complete)
  mx = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
  const float nan = __int_as_float(0x7fc00000);
  if (nans > 0 || !(mx > -INFINITY && mx < INFINITY)) {   // (uniform) a NaN, +inf or all -inf: token_scores_kernel's rows of NaN
    if (tid < 4) o[tid] = nan;
    return;
  }
  // K: the key of the top_k-th largest entry = the largest T with #{key_i >= T} >= top_k, by bisection over the key space with integer
  // block counts (-inf entries count, as in the sampler's select); everything >= it is kept (ties included), -inf never
  unsigned thr = 0u;
  if (!greedy && top_k > 0 && top_k < V) {
    unsigned lo = 0u, hi = 0xffffffffu;
    while (lo < hi) {   // uniform: every thread holds the same counts
      const unsigned mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1u);
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < KPT; ++q) cnt += key[q] >= mid ? 1 : 0;
      if (block_sum_i32(cnt, s_c, lane, wv) >= top_k) lo = mid; else hi = mid - 1u;
    }
    thr = lo;
  }
  // e_i = exp(l_i - max) in fp64, the subtraction in fp32; from here on v / e hold the KEPT entries only (-inf / 0 elsewhere)
  float v[KPT];
  double e[KPT];
  double za = 0.0, zk = 0.0;
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const float l = key2f(key[q]);
    const double ea = l > -INFINITY ? exp((double)(l - mx)) : 0.0;   // (NaN entries and the slots past the row: 0)
    const bool kept = l > -INFINITY && key[q] >= thr;
    za += ea;
    e[q] = kept ? ea : 0.0;
    v[q] = kept ? l : -INFINITY;
    zk += e[q];
  }
  const double all = block_sum_f64(za, s_w, lane, wv);
  // S: the kept tokens not below tau, the smallest value whose mass G of kept tokens not above it exceeds the cut (the sampler's general
  // path: bisection over the key space, each round one fixed-order fp64 block sum).  Keys decode to floats for the comparison: float order
  // is nkey order (-0.0 folded onto +0.0), and no round looks above the maximum, which always survives
  float tauf = -INFINITY;
  if (!greedy && top_p < 1.0f) {
    const double Z = block_sum_f64(zk, s_w, lane, wv);
    const double cut = (1.0 - (double)top_p) * Z;
    unsigned lo = 0u, hi = f2key(mx);
    if (!(Z > cut)) lo = hi;   // top_p = 0: the maximum alone
    while (lo < hi) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      const float midf = key2f(mid);
      double m = 0.0;
#pragma unroll
      for (int q = 0; q < KPT; ++q) m += v[q] <= midf ? e[q] : 0.0;
      if (block_sum_f64(m, s_w, lane, wv) > cut) hi = mid; else lo = mid + 1u;
    }
    tauf = key2f(lo);
  }
  double sp = 0.0, tp = 0.0;
  int np = 0;
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    const bool in = v[q] > -INFINITY && v[q] >= tauf;
    if (in && e[q] > 0.0) { sp += e[q]; tp = fma(e[q], (double)(v[q] - mx), tp); }
    np += in ? 1 : 0;
  }
  const double s = block_sum_f64(sp, s_w, lane, wv);
  const double t = block_sum_f64(tp, s_w, lane, wv);
  const int n = block_sum_i32(np, s_c, lane, wv);
  if (tid == 0) {
    const double ls = log(s);
    float lp = nan;
    if (tok >= 0 && tok < V) {
      float l = row[tok];
      if (scale) l = l / temperature;   // (the same IEEE division: the bits of the entry above)
      lp = (l > -INFINITY && f2key(l) >= thr && l >= tauf) ? (float)((double)(l - mx) - ls) : -INFINITY;
    }
    o[0] = lp;
    o[1] = (float)(ls - t / s);
    o[2] = (float)(ls - log(all));   // (nothing filtered: s and all are the same terms in the same order, exactly 0)
    o[3] = (float)n;
  }
}

template <int KPT>
__global__ __launch_bounds__(256) void filtered_scores_kernel(const float* __restrict__ logits, int V, const StepState* __restrict__ state,
                                                              const int64_t* __restrict__ ids, long ids_stride, int L0, int forced_period, int top_k,
                                                              float temperature, float top_p, int greedy, float* __restrict__ out, int cols) {
  const int j = state->j;
  if (j < 1 || j > cols) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  float* o = out + ((long)b * cols + (j - 1)) * 4;
  if (forced_period > 0 && j % forced_period == 0) {
    if (tid < 4) o[tid] = 0.f;
    return;
  }
  __shared__ double s_w[4];
  __shared__ int s_c[4];
  __shared__ float s_f[4];
  filtered_scores_row<KPT>(logits + (long)b * V, V, ids[(long)b * ids_stride + L0 + (j - 1)], top_k, temperature, top_p, greedy != 0, o, s_w, s_c, s_f);
}

int launch_filtered_scores(const float* logits, int V, const StepState* state, const int64_t* ids, long ids_stride, int L0, int forced_period, int top_k,
                           float temperature, float top_p, bool greedy, float* out, int cols, int B, hipStream_t st) {
  if (B <= 0 || cols <= 0) return 0;
  if (!logits || !ids || !out || V < 1 || V > 256 * 72 || !(temperature > 0.0f) || !(top_p >= 0.0f && top_p <= 1.0f)) return (int)hipErrorInvalidValue;
  if (V <= 256 * 36)
    hipLaunchKernelGGL(filtered_scores_kernel<36>, dim3(B), dim3(256), 0, st, logits, V, state, ids, ids_stride, L0, forced_period, top_k, temperature, top_p,
                       greedy ? 1 : 0, out, cols);
  else
    hipLaunchKernelGGL(filtered_scores_kernel<72>, dim3(B), dim3(256), 0, st, logits, V, state, ids, ids_stride, L0, forced_period, top_k, temperature, top_p,
                       greedy ? 1 : 0, out, cols);
  return (int)hipGetLastError();
}

static std::atomic<long long> g_filtered_scores_launches{0};
void filtered_scores_note(int launches) { g_filtered_scores_launches += launches; }
long long filtered_scores_launches() { return g_filtered_scores_launches.load(); }

// ------------------------------------------------------------------------------------------------ eval heads
// Shifted cross-entropy of teacher-forced logits (HF ForCausalLM loss, train_gpt.py:356-376): row r = (b, l) of a chunk of logits
// [rows][V] fp32 predicts labels[b][l + 1]; nll[r] = logsumexp(logits[r]) - logits[r][target], 0 where the target is -100 (or l is
// the last position).  One workgroup per row, fixed-order reductions.
// nll of one logits row against `tgt`, by the whole workgroup (the value is valid in thread 0); red: 8 floats of LDS
__device__ __forceinline__ float ce_row_nll(const float* __restrict__ row, long tgt, int V, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 256) mx = fmaxf(mx, row[i]);
  mx = wave_max(mx);
  if (lane == 0) red[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int i = tid; i < V; i += 256) sum += expf(row[i] - mx);
  sum = wave_sum(sum);
  if (lane == 0) red[4 + wv] = sum;
  __syncthreads();
  return logf((red[4] + red[5]) + (red[6] + red[7])) + mx - row[tgt];
}

__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long row0,
                                                      int L, int V, float* __restrict__ nll) {
  __shared__ float red[8];
  const long r = row0 + blockIdx.x;
  const int l = (int)(r % L), tid = threadIdx.x;
  const long tgt = l + 1 < L ? labels[r + 1] : -100;
  if (tgt < 0 || tgt >= V) { if (tid == 0) nll[r] = 0.f; return; }
  const float v = ce_row_nll(logits + (long)blockIdx.x * V, tgt, V, red);
  if (tid == 0) nll[r] = v;
}

// The same per row of a chunk of teacher-forced rows whose targets are given ids (ivg_kv_extend): chunk row i is row r = row0 + i of
// [B][Tc] rows, (b, c) = (r / Tc, r % Tc); its target is ids[b][c] (ids already points at the column after the row's own token) and its
// nll goes to out[b * out_ld + c]
__global__ __launch_bounds__(256) void token_nll_kernel(const float* __restrict__ logits, const int64_t* __restrict__ ids, long ids_stride,
                                                        long row0, int Tc, int V, float* __restrict__ out, long out_ld) {
  __shared__ float red[8];
  const long r = row0 + blockIdx.x;
  const long b = r / Tc, c = r - b * Tc;
  const long tgt = ids[b * ids_stride + c];
  if (tgt < 0 || tgt >= V) { if (threadIdx.x == 0) out[b * out_ld + c] = 0.f; return; }
  const float v = ce_row_nll(logits + (long)blockIdx.x * V, tgt, V, red);
  if (threadIdx.x == 0) out[b * out_ld + c] = v;
}

int launch_token_nll(const float* logits, const int64_t* ids, long ids_stride, long row0, int rows, int Tc, int V, float* out, long out_ld,
                     hipStream_t st) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(token_nll_kernel, dim3((unsigned)rows), dim3(256), 0, st, logits, ids, ids_stride, row0, Tc, V, out, out_ld);
  return (int)hipGetLastError();
}

int launch_ce_rows(const float* logits, const int64_t* labels, long row0, int rows, int L, int V, float* nll, hipStream_t st) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, logits, labels, row0, L, V, nll);
  return (int)hipGetLastError();
}

// out[b] = { sum_l nll[b][l], number of positions l whose target labels[b][l + 1] is not ignored }
__global__ __launch_bounds__(256) void ce_reduce_kernel(const float* __restrict__ nll, const int64_t* __restrict__ labels, int L, int V,
                                                        float* __restrict__ out) {
  __shared__ float rs[4], rc[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  float s = 0.f, c = 0.f;
  for (int l = tid; l + 1 < L; l += 256) {
    const long t = labels[(long)b * L + l + 1];
    if (t >= 0 && t < V) { s += nll[(long)b * L + l]; c += 1.f; }
  }
  s = wave_sum(s); c = wave_sum(c);
  if ((tid & 63) == 0) { rs[tid >> 6] = s; rc[tid >> 6] = c; }
  __syncthreads();
  if (tid == 0) { out[2 * b] = (rs[0] + rs[1]) + (rs[2] + rs[3]); out[2 * b + 1] = (rc[0] + rc[1]) + (rc[2] + rc[3]); }
}

int launch_ce_reduce(const float* nll, const int64_t* labels, int B, int L, int V, float* out, hipStream_t st) {
  if (B <= 0) return 0;
  hipLaunchKernelGGL(ce_reduce_kernel, dim3((unsigned)B), dim3(256), 0, st, nll, labels, L, V, out);
  return (int)hipGetLastError();
}

// action reconstruction error (action_model.py:187-196): every position p >= prelude of trajectory b predicts the action of its
// frame slot i = (p - prelude) / 17, a_hat = W h[b][p] + bias; out[b] = sum over positions and action dims of (a_hat - a)^2.
template <typename T>
__global__ __launch_bounds__(256) void action_recon_kernel(const T* __restrict__ hidden, const float* __restrict__ W, const float* __restrict__ bias,
                                                           const float* __restrict__ act, int L, int H, int A, int act_T, int ctx, int prelude,
                                                           float* __restrict__ out) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float err = 0.f;   // lane 0 of every wave accumulates the positions that wave handles (fixed order)
  for (int p = prelude + wv; p < L; p += 4) {
    const int slot = (p - prelude) / 17;
    const T* h = hidden + ((long)b * L + p) * H;
    for (int a = 0; a < A; ++a) {
      float s = 0.f;
      for (int c = lane; c < H; c += 64) s = fmaf(to_f32(h[c]), W[(long)a * H + c], s);
      s = wave_sum(s);
      const float d = s + bias[a] - act[((long)b * act_T + ctx - 1 + slot) * A + a];
      err = fmaf(d, d, err);
    }
  }
  if (lane == 0) red[wv] = err;
  __syncthreads();
  if (tid == 0) out[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

int launch_action_recon(const void* hidden, const float* W, const float* bias, const float* act, int B, int L, int H, int A, int act_T,
                        int ctx, int prelude, float* out, DType dt, hipStream_t st) {
  if (B <= 0) return 0;
  if (dt == BF16) hipLaunchKernelGGL(action_recon_kernel<bf16_t>, dim3((unsigned)B), dim3(256), 0, st, (const bf16_t*)hidden, W, bias, act, L, H, A, act_T, ctx, prelude, out);
  else hipLaunchKernelGGL(action_recon_kernel<float>, dim3((unsigned)B), dim3(256), 0, st, (const float*)hidden, W, bias, act, L, H, A, act_T, ctx, prelude, out);
  return (int)hipGetLastError();
}

// flag[0] += number of 4-byte words that differ between rows of a and b (row r at a + r * a_stride bytes; row_bytes % 4 == 0).
// Used to verify that a kept KV cache was built from exactly the prefix a step-wise caller presents again.
__global__ __launch_bounds__(256) void compare_rows_kernel(const unsigned* __restrict__ a, long a_stride, const unsigned* __restrict__ b,
                                                           long b_stride, long row_words, int* __restrict__ flag) {
  const int r = blockIdx.y;
  const unsigned* pa = (const unsigned*)((const char*)a + (long)r * a_stride);
  const unsigned* pb = (const unsigned*)((const char*)b + (long)r * b_stride);
  int bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < row_words; i += (long)gridDim.x * 256) bad += pa[i] != pb[i] ? 1 : 0;
  bad = (int)wave_sum((float)bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(flag, bad);
}

int launch_compare_rows(const void* a, long a_stride_bytes, const void* b, long b_stride_bytes, int rows, long row_bytes, int* flag,
                        hipStream_t st) {
  if (rows <= 0 || row_bytes <= 0) return 0;
  if (row_bytes % 4 != 0 || a_stride_bytes % 4 != 0 || b_stride_bytes % 4 != 0) return (int)hipErrorInvalidValue;
  const long words = row_bytes / 4;
  const unsigned gx = (unsigned)std::min<long>(64, (words + 255) / 256);
  hipLaunchKernelGGL(compare_rows_kernel, dim3(gx, (unsigned)rows), dim3(256), 0, st, (const unsigned*)a, a_stride_bytes,
                     (const unsigned*)b, b_stride_bytes, words, flag);
  return (int)hipGetLastError();
}

}  // namespace ivg
