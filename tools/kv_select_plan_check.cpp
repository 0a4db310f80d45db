// Stand-alone host check of ivg_kv_select's move planner (ivideogpt_amd/csrc/kv_select_plan.h): random parents maps, the plan executed
// on a simulated buffer in the order launch_kv_select uses (staged rows out, direct rows in place, staged rows back in) against a
// gather from a snapshot.  CPU only; build with the sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kv_select_plan_check.cpp -o kv_select_plan_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ivideogpt_amd/csrc/kv_select_plan.h"

using namespace ivg;

static int fail(const char* what, int chunk, int B_old, int n) {
  std::fprintf(stderr, "FAIL: %s (chunk %d, B_old %d, n %d)\n", what, chunk, B_old, n);
  return 1;
}

static int check(const std::vector<int32_t>& parents, int B_old, int chunk) {
  const int n = (int)parents.size();
  KvSelectPlan plan;
  if (kv_select_plan(parents.data(), n, B_old, chunk, &plan) != KV_PLAN_OK) return fail("a valid map was refused", chunk, B_old, n);
  std::vector<int> rows(chunk), snap, scratch(plan.n_staged), written(chunk, 0);
  for (int r = 0; r < chunk; ++r) rows[r] = 1000 + r;
  snap = rows;
  int moved = 0;
  for (int i = 0; i < n; ++i) moved += parents[i] != i;
  if (plan.n_direct + plan.n_staged != moved) return fail("moves != rows with parents[i] != i", chunk, B_old, n);
  // direct launch: no destination is a source of the same launch, destinations are distinct
  std::vector<int> is_dst(chunk, 0);
  for (int k = 0; k < plan.n_direct; ++k) {
    if (plan.direct.dst[k] >= n || plan.direct.src[k] >= B_old) return fail("direct move out of range", chunk, B_old, n);
    if (is_dst[plan.direct.dst[k]]++) return fail("two direct moves write one row", chunk, B_old, n);
  }
  for (int k = 0; k < plan.n_direct; ++k)
    if (is_dst[plan.direct.src[k]]) return fail("a direct move reads a row a direct move writes", chunk, B_old, n);
  for (int k = 0; k < plan.n_staged; ++k) {
    if (plan.staged.dst[k] >= n || plan.staged.src[k] >= B_old) return fail("staged move out of range", chunk, B_old, n);
    if (is_dst[plan.staged.dst[k]]++) return fail("two moves write one row", chunk, B_old, n);
  }
  for (int k = 0; k < plan.n_staged; ++k) scratch[k] = rows[plan.staged.src[k]];
  for (int k = 0; k < plan.n_direct; ++k) { rows[plan.direct.dst[k]] = rows[plan.direct.src[k]]; ++written[plan.direct.dst[k]]; }
  for (int k = 0; k < plan.n_staged; ++k) { rows[plan.staged.dst[k]] = scratch[k]; ++written[plan.staged.dst[k]]; }
  for (int r = 0; r < chunk; ++r) {
    const int want = r < n ? snap[parents[r]] : snap[r];
    if (rows[r] != want) return fail("result differs from the gather of the snapshot", chunk, B_old, n);
    if (written[r] != (r < n && parents[r] != r ? 1 : 0)) return fail("a row that does not move was written (or a moved one twice)", chunk, B_old, n);
  }
  return 0;
}

int main() {
  std::mt19937 rng(20240611);
  long cases = 0;
  for (int chunk : {1, 2, 3, 8, 17, 64, 127, 128})
    for (int rep = 0; rep < 4000; ++rep) {
      const int B_old = 1 + (int)(rng() % chunk), n = 1 + (int)(rng() % chunk);
      std::vector<int32_t> p(n);
      const int kind = rng() % 5;
      for (int i = 0; i < n; ++i) {
        if (kind == 0) p[i] = (int32_t)(rng() % B_old);                                  // anything
        else if (kind == 1) p[i] = i < B_old ? i : (int32_t)(rng() % B_old);             // survivors in place, growth
        else if (kind == 2) p[i] = (int32_t)((i + 1) % B_old);                           // cyclic shift
        else if (kind == 3) p[i] = (int32_t)(B_old - 1);                                 // one row everywhere
        else p[i] = (rng() & 1) && i < B_old ? i : (int32_t)(rng() % B_old);             // half fixed
      }
      if (check(p, B_old, chunk)) return 1;
      ++cases;
    }
  // refusals write nothing
  KvSelectPlan plan; plan.n_direct = -7;
  const int32_t bad[3] = {0, 3, 1}, neg[2] = {0, -1}, ok[3] = {0, 1, 2};
  if (kv_select_plan(bad, 3, 3, 8, &plan) != KV_PLAN_INVALID || kv_select_plan(neg, 2, 3, 8, &plan) != KV_PLAN_INVALID ||
      kv_select_plan(ok, 0, 3, 8, &plan) != KV_PLAN_INVALID || kv_select_plan(ok, 3, 3, 2, &plan) != KV_PLAN_INVALID ||
      kv_select_plan(ok, 3, 2, 2, &plan) != KV_PLAN_CAPACITY || kv_select_plan(ok, 3, 3, 129, &plan) != KV_PLAN_INVALID ||
      kv_select_plan(nullptr, 3, 3, 8, &plan) != KV_PLAN_INVALID || plan.n_direct != -7)
    return fail("a refusal", 0, 0, 0);
  if (kv_select_plan(ok, 3, 3, 8, &plan) != KV_PLAN_OK || plan.n_direct != 0 || plan.n_staged != 0) return fail("the identity moves rows", 8, 3, 3);
  std::printf("kv_select_plan: %ld random maps and the refusals ok\n", cases);
  return 0;
}
