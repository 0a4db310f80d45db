// ivg_kv_select / ivg_cache_select: trajectory rows of a buffer gathered by a parents map (HF's _reorder_cache on the kept K / V cache;
// DESIGN.md 3.6).  A strided copy in 16-byte vectors: plain loads and stores, no atomics, no LDS; the move list travels as a by-value
// kernel argument (kv_select_plan.h builds it).
#include <algorithm>
#include "ops.h"

namespace ivg {

// where the rows of one side of a copy are: a buffer of the caller's layout (row = the move's table entry) or the dense scratch of
// the staged rows (row = the move's index)
struct KvSide {
  char* base;
  long slab_stride, row_stride, head_stride, plane_b;
  int table;
};

constexpr int GATHER_THREADS = 256, GATHER_UNROLL = 4;   // 16 KiB of 16-byte vectors per workgroup, four loads in flight per lane

// grid (ranges of GATHER_THREADS * GATHER_UNROLL vectors, move * heads + head, slab).  Of every (row, head) block the first vec_a
// vectors move and, from plane_b on, vec_b more; nothing else of either side is touched
template <typename V>
__global__ __launch_bounds__(GATHER_THREADS) void kv_gather_rows_kernel(KvSide src, KvSide dst, KvMoves mv, int heads, int vec_a, int vec_b) {
  const int m = blockIdx.y / heads, h = blockIdx.y % heads;
  const long s_row = src.table ? (long)mv.src[m] : (long)m, d_row = dst.table ? (long)mv.dst[m] : (long)m;
  const char* sp = src.base + blockIdx.z * src.slab_stride + s_row * src.row_stride + h * src.head_stride;
  char* dp = dst.base + blockIdx.z * dst.slab_stride + d_row * dst.row_stride + h * dst.head_stride;
  const int nv = vec_a + vec_b;
  const int v0 = blockIdx.x * (GATHER_THREADS * GATHER_UNROLL) + threadIdx.x;
  V r[GATHER_UNROLL];
#pragma unroll
  for (int k = 0; k < GATHER_UNROLL; ++k) {
    const int v = v0 + k * GATHER_THREADS;
    if (v < nv) r[k] = *(const V*)(sp + (v < vec_a ? (long)v * sizeof(V) : src.plane_b + (long)(v - vec_a) * sizeof(V)));
  }
#pragma unroll
  for (int k = 0; k < GATHER_UNROLL; ++k) {
    const int v = v0 + k * GATHER_THREADS;
    if (v < nv) *(V*)(dp + (v < vec_a ? (long)v * sizeof(V) : dst.plane_b + (long)(v - vec_a) * sizeof(V))) = r[k];
  }
}

static int launch_gather(const KvSide& src, const KvSide& dst, const KvMoves& mv, int n_moves, int slabs, int heads, long bytes_a, long bytes_b,
                         int vec, hipStream_t st) {
  if (n_moves <= 0 || slabs <= 0) return 0;
  const int va = (int)(bytes_a / vec), vb = (int)(bytes_b / vec);
  if (va + vb <= 0) return 0;
  const dim3 grid(cdiv(va + vb, GATHER_THREADS * GATHER_UNROLL), n_moves * heads, slabs);
  if (vec == 16) hipLaunchKernelGGL(kv_gather_rows_kernel<Chunk16>, grid, dim3(GATHER_THREADS), 0, st, src, dst, mv, heads, va, vb);
  else hipLaunchKernelGGL(kv_gather_rows_kernel<uint32_t>, grid, dim3(GATHER_THREADS), 0, st, src, dst, mv, heads, va, vb);
  return (int)hipGetLastError();
}

int launch_kv_select(const KvSelectBuf& b, const KvSelectPlan& plan, void* scratch, size_t scratch_bytes, hipStream_t st) {
  if (plan.n_direct + plan.n_staged == 0 || b.slabs <= 0 || b.bytes_a + b.bytes_b <= 0) return 0;
  if (!b.base || (b.vec != 16 && b.vec != 4) || b.heads <= 0 || b.slabs > 65535 || (long)KV_SELECT_MAX_ROWS * b.heads > 65535) return (int)hipErrorInvalidValue;
  const long al = b.vec - 1;
  if ((((uintptr_t)b.base | (uintptr_t)scratch) & al) || ((b.slab_stride | b.row_stride | b.head_stride | b.bytes_a | b.bytes_b | b.plane_b) & al) ||
      (b.bytes_a + b.bytes_b) / b.vec > (long)INT32_MAX / 2)
    return (int)hipErrorInvalidValue;
  const size_t seg = (size_t)(b.bytes_a + b.bytes_b), per_slab = b.staged_bytes_per_slab(plan.n_staged);
  int group = b.slabs;   // slabs whose staged rows the scratch holds at once
  if (plan.n_staged > 0) {
    if (!scratch || per_slab > scratch_bytes) return -4;
    group = (int)std::min<size_t>((size_t)b.slabs, scratch_bytes / per_slab);
  }
  const KvSide dense{(char*)scratch, (long)per_slab, (long)((size_t)b.heads * seg), (long)seg, b.bytes_a, 0};
  for (int s0 = 0; s0 < b.slabs; s0 += group) {
    const int ns = std::min(group, b.slabs - s0);
    const KvSide rows{b.base + (size_t)s0 * b.slab_stride, b.slab_stride, b.row_stride, b.head_stride, b.plane_b, 1};
    // every staged source is read before the direct moves (which may overwrite it) run; every direct source is neither a direct nor
    // a staged destination, so the order of the last two launches does not matter
    if (int rc = launch_gather(rows, dense, plan.staged, plan.n_staged, ns, b.heads, b.bytes_a, b.bytes_b, b.vec, st)) return rc;
    if (int rc = launch_gather(rows, rows, plan.direct, plan.n_direct, ns, b.heads, b.bytes_a, b.bytes_b, b.vec, st)) return rc;
    if (int rc = launch_gather(dense, rows, plan.staged, plan.n_staged, ns, b.heads, b.bytes_a, b.bytes_b, b.vec, st)) return rc;
  }
  return 0;
}

int launch_gather_rows_by_parent(const void* src, void* dst, long row_bytes, const int32_t* parents, int n, hipStream_t st) {
  if (n <= 0 || row_bytes <= 0) return 0;
  if (!src || !dst || !parents || (row_bytes & 15) || (((uintptr_t)src | (uintptr_t)dst) & 15) || row_bytes / 16 > (long)INT32_MAX / 2) return (int)hipErrorInvalidValue;
  for (int i = 0; i < n; ++i)
    if (parents[i] < 0) return (int)hipErrorInvalidValue;
  for (int i0 = 0; i0 < n;) {   // runs of consecutive destination rows whose sources lie in one window of 256 rows
    const int win = parents[i0] / 256;
    KvMoves mv{};
    int k = 0;
    while (i0 + k < n && k < KV_SELECT_MAX_ROWS && parents[i0 + k] / 256 == win) { mv.src[k] = (uint8_t)(parents[i0 + k] % 256); ++k; }
    const KvSide s{(char*)src + (size_t)win * 256 * row_bytes, 0, row_bytes, 0, 0, 1};
    const KvSide d{(char*)dst + (size_t)i0 * row_bytes, 0, row_bytes, 0, 0, 0};
    if (int rc = launch_gather(s, d, mv, k, 1, 1, row_bytes, 0, 16, st)) return rc;
    i0 += k;
  }
  return 0;
}

// ivg_kv_snapshot_create / _restore: the rows of b against their compact image dense = [slabs][dense_rows][heads]{bytes_a | bytes_b}.
// The image is the dense side of the gather kernel; for a restore it is a table side too, indexed by parents through the move list
int launch_kv_snapshot(const KvSelectBuf& b, void* dense, int dense_rows, const int32_t* parents, int n, bool restore, hipStream_t st) {
  if (n <= 0 || b.slabs <= 0 || b.bytes_a + b.bytes_b <= 0) return 0;
  if (!b.base || !dense || (b.vec != 16 && b.vec != 4) || b.heads <= 0 || b.slabs > 65535 || (long)KV_SELECT_MAX_ROWS * b.heads > 65535 ||
      dense_rows <= 0 || dense_rows > 256 || n > 256 || (!restore && n != dense_rows) || (restore && !parents))
    return (int)hipErrorInvalidValue;
  const long al = b.vec - 1;
  if ((((uintptr_t)b.base | (uintptr_t)dense) & al) || ((b.slab_stride | b.row_stride | b.head_stride | b.bytes_a | b.bytes_b | b.plane_b) & al) ||
      (b.bytes_a + b.bytes_b) / b.vec > (long)INT32_MAX / 2)
    return (int)hipErrorInvalidValue;
  if (restore)
    for (int i = 0; i < n; ++i)
      if (parents[i] < 0 || parents[i] >= dense_rows) return (int)hipErrorInvalidValue;
  const long seg = b.bytes_a + b.bytes_b, drow = (long)b.heads * seg;
  const KvSide rows{b.base, b.slab_stride, b.row_stride, b.head_stride, b.plane_b, 1};
  for (int i0 = 0; i0 < n; i0 += KV_SELECT_MAX_ROWS) {   // cache rows [i0, i0 + k)
    const int k = std::min(KV_SELECT_MAX_ROWS, n - i0);
    KvMoves mv{};
    for (int m = 0; m < k; ++m) { mv.src[m] = (uint8_t)(restore ? parents[i0 + m] : i0 + m); mv.dst[m] = (uint8_t)(i0 + m); }
    const KvSide image{(char*)dense + (restore ? 0 : (size_t)i0 * drow), (long)dense_rows * drow, drow, seg, b.bytes_a, restore ? 1 : 0};
    if (int rc = restore ? launch_gather(image, rows, mv, k, b.slabs, b.heads, b.bytes_a, b.bytes_b, b.vec, st)
                         : launch_gather(rows, image, mv, k, b.slabs, b.heads, b.bytes_a, b.bytes_b, b.vec, st))
      return rc;
  }
  return 0;
}

static std::atomic<long long> g_kv_snapshot_rows[2] = {{0}, {0}};
void kv_snapshot_note(int saved, int restored) { g_kv_snapshot_rows[0] += saved; g_kv_snapshot_rows[1] += restored; }
long long kv_snapshot_rows(int restored) { return g_kv_snapshot_rows[restored ? 1 : 0].load(); }

static std::atomic<long long> g_kv_select_rows[2] = {{0}, {0}};
void kv_select_note(int direct, int staged) { g_kv_select_rows[0] += direct; g_kv_select_rows[1] += staged; }
long long kv_select_rows(int staged) { return g_kv_select_rows[staged ? 1 : 0].load(); }

}  // namespace ivg
