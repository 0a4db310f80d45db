// The move planner of ivg_kv_select (kv_select.hip has the kernel, DESIGN.md 3.6 the contract).  Plain C++: no HIP, no engine -- it is
// also compiled into a stand-alone host program under the address and undefined-behaviour sanitizers (tools/kv_select_plan_check.cpp).
//
// "new row i := old row parents[i], 0 <= i < n" over B_old rows, as if gathered from a snapshot.  Rows with parents[i] == i do not move.
// Every other row is one move (dst i, src parents[i]) of one of two kinds:
//   direct  the source row is not overwritten by this select: it stays where it is (parents[src] == src, src < n) or is dropped
//           (src >= n).  Copied in place, cache -> cache: destinations are distinct and no destination is a source of a direct move.
//   staged  the source row is itself a destination.  Copied out to scratch first (slot k of the staged list) and back in after the
//           direct moves, so every source is read before any launch of the select writes it.
#pragma once
#include <cstdint>

namespace ivg {

constexpr int KV_SELECT_MAX_ROWS = 128;   // the cache chunk's limit: a move list fits a by-value kernel argument

struct KvMoves { uint8_t src[KV_SELECT_MAX_ROWS]; uint8_t dst[KV_SELECT_MAX_ROWS]; };

struct KvSelectPlan {
  KvMoves direct, staged;
  int n_direct = 0, n_staged = 0;
};

enum { KV_PLAN_OK = 0, KV_PLAN_INVALID = -1, KV_PLAN_CAPACITY = -4 };

// chunk: rows the buffer has room for.  Writes *out only on KV_PLAN_OK
inline int kv_select_plan(const int32_t* parents, int n, int B_old, int chunk, KvSelectPlan* out) {
  if (!parents || !out || n <= 0 || B_old <= 0 || chunk <= 0 || chunk > KV_SELECT_MAX_ROWS || B_old > chunk) return KV_PLAN_INVALID;
  if (n > chunk) return KV_PLAN_CAPACITY;
  for (int i = 0; i < n; ++i)
    if (parents[i] < 0 || parents[i] >= B_old) return KV_PLAN_INVALID;
  KvSelectPlan p;
  for (int i = 0; i < n; ++i) {
    const int s = parents[i];
    if (s == i) continue;
    const bool src_kept = s >= n || parents[s] == s;   // nothing of this select writes row s
    KvMoves& m = src_kept ? p.direct : p.staged;
    int& k = src_kept ? p.n_direct : p.n_staged;
    m.src[k] = (uint8_t)s; m.dst[k] = (uint8_t)i;
    ++k;
  }
  for (int k = p.n_direct; k < KV_SELECT_MAX_ROWS; ++k) p.direct.src[k] = p.direct.dst[k] = 0;
  for (int k = p.n_staged; k < KV_SELECT_MAX_ROWS; ++k) p.staged.src[k] = p.staged.dst[k] = 0;
  *out = p;
  return KV_PLAN_OK;
}

}  // namespace ivg
