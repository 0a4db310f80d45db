// The switch table of libivg (switches.h): read from the environment, published through one atomic pointer.
#include "switches.h"

#include <atomic>
#include <cstdlib>
#include <mutex>

namespace ivg {

static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return (v && v[0]) ? atoi(v) : dflt;
}

// One row per switch; read_env and operator== are loops over it.
enum Class { POLICY, DEV };              // DEV: a development (A/B) switch, inert without IVG_DEV=1
enum Norm { NONZERO, IS_ONE, RANGE };    // raw value -> field: v != 0, v == 1, or v itself inside [lo, hi] (else the default)
struct Row { const char* env; int Switches::*field; int dflt; Class cls; Norm norm; int lo, hi; };
static const Row kRows[] = {
  {"IVG_GRAPH", &Switches::graph, 0, POLICY, IS_ONE},
  {"IVG_DECODE_LDS_KB", &Switches::decode_lds_kb, 160, POLICY, RANGE, 16, 160},
  {"IVG_CONV3X3", &Switches::conv3x3, 1, DEV, NONZERO},
  {"IVG_SUBPIXEL", &Switches::subpixel, 1, DEV, NONZERO},
  {"IVG_GEMM256", &Switches::gemm256, 1, DEV, NONZERO},
  {"IVG_GEMM256X3", &Switches::gemm256x3, 1, DEV, NONZERO},
  {"IVG_KV24", &Switches::kv24, 1, DEV, NONZERO},
  {"IVG_DG3", &Switches::dg3, 1, DEV, NONZERO},
  {"IVG_FLASH_PREFILL", &Switches::flash_prefill, 1, DEV, NONZERO},
  {"IVG_KV_EXTEND_CHUNK", &Switches::kv_extend_chunk, 1, DEV, NONZERO},
  {"IVG_GN_APPLY_FUSE", &Switches::gn_apply_fuse, 1, DEV, NONZERO},
  {"IVG_X3", &Switches::x3, 1, DEV, NONZERO},
  {"IVG_CONV_CAP", &Switches::conv_cap, 0, DEV, IS_ONE},
  {"IVG_DECODE_ATTN_WINDOW", &Switches::decode_attn_window, 1, DEV, NONZERO},
};
static_assert(sizeof(Switches) == sizeof(kRows) / sizeof(kRows[0]) * sizeof(int), "a field of Switches without a row (or a row too many)");

static Switches read_env() {
  Switches s{};
  const bool dev = env_int("IVG_DEV", 0) == 1;
  for (const Row& r : kRows) {
    const int v = (r.cls == DEV && !dev) ? r.dflt : env_int(r.env, r.dflt);
    s.*r.field = r.norm == NONZERO ? v != 0 : r.norm == IS_ONE ? v == 1 : (v >= r.lo && v <= r.hi) ? v : r.dflt;
  }
  return s;
}

bool Switches::operator==(const Switches& o) const {
  for (const Row& r : kRows)
    if (this->*r.field != o.*r.field) return false;
  return true;
}

// A reload that CHANGES the table publishes a new immutable one through one atomic pointer and never frees or rewrites the old
// (a launcher on another host thread may hold a reference for the length of a launch; ~64 bytes per change, deliberately leaked).
// A reload that reads the same values publishes nothing and leaves the generation alone: ivg_create re-reads the environment, and
// with the generation in the key of captured step graphs every engine construction (replicas, capacity growth) would otherwise
// orphan the graphs of all live engines (advice, round 5).  getenv() is only called here, under the mutex -- a Python thread
// changing os.environ while another thread reloads is the caller's race (ivideogpt_amd/switches.py).
static std::atomic<const Switches*> g_cur{nullptr};
static std::atomic<unsigned> g_gen{0};
static std::mutex g_mu;

void reload_switches() {
  std::lock_guard<std::mutex> lk(g_mu);
  const Switches now = read_env();
  const Switches* cur = g_cur.load(std::memory_order_acquire);
  if (cur && *cur == now) return;
  g_cur.store(new Switches(now), std::memory_order_release);
  g_gen.fetch_add(1, std::memory_order_release);
}

const Switches& sw() {
  const Switches* p = g_cur.load(std::memory_order_acquire);
  if (!p) { reload_switches(); p = g_cur.load(std::memory_order_acquire); }
  return *p;
}

unsigned switches_generation() { return g_gen.load(std::memory_order_acquire); }

}  // namespace ivg
