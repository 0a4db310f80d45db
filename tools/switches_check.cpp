// Stand-alone host check of libivg's switch table (ivideogpt_amd/csrc/switches.cpp): documented defaults, the IVG_DEV gate of the
// development switches, the normalisations, the generation rule of reload_switches() and the retired names.  CPU only; build with
// the sanitizers and run with leak detection off (a reload that changes the table leaks the old one by design):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/switches_check.cpp -o switches_check
//   ASAN_OPTIONS=detect_leaks=0 ./switches_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ivideogpt_amd/csrc/switches.cpp"

using namespace ivg;

extern char** environ;

// The documented table (switches.h's comment), written out again on purpose: name, field, default, a raw value that selects the
// other arm and the field's value there.
struct Doc { const char* env; int Switches::*field; int dflt; bool dev; const char* other; int other_val; };
static const Doc kDoc[] = {
  {"IVG_GRAPH", &Switches::graph, 0, false, "1", 1},
  {"IVG_DECODE_LDS_KB", &Switches::decode_lds_kb, 160, false, "40", 40},
  {"IVG_CONV3X3", &Switches::conv3x3, 1, true, "0", 0},
  {"IVG_SUBPIXEL", &Switches::subpixel, 1, true, "0", 0},
  {"IVG_GEMM256", &Switches::gemm256, 1, true, "0", 0},
  {"IVG_GEMM256X3", &Switches::gemm256x3, 1, true, "0", 0},
  {"IVG_KV24", &Switches::kv24, 1, true, "0", 0},
  {"IVG_DG3", &Switches::dg3, 1, true, "0", 0},
  {"IVG_FLASH_PREFILL", &Switches::flash_prefill, 1, true, "0", 0},
  {"IVG_KV_EXTEND_CHUNK", &Switches::kv_extend_chunk, 1, true, "0", 0},
  {"IVG_GN_APPLY_FUSE", &Switches::gn_apply_fuse, 1, true, "0", 0},
  {"IVG_X3", &Switches::x3, 1, true, "0", 0},
  {"IVG_CONV_CAP", &Switches::conv_cap, 0, true, "1", 1},
  {"IVG_DECODE_ATTN_WINDOW", &Switches::decode_attn_window, 1, true, "0", 0},
};
static const int kDocN = sizeof(kDoc) / sizeof(kDoc[0]);
static_assert(sizeof(Switches) == kDocN * sizeof(int), "kDoc names every field of Switches");

// retired in round 7, each with the value that used to select its other arm
static const char* const kRetired[][2] = {
  {"IVG_GN_FUSE", "0"}, {"IVG_FLASH_XATT", "0"}, {"IVG_DG3_WARM", "0"}, {"IVG_WARM_GATE_UP", "1"}, {"IVG_DECODE_W_SHARED", "0"},
  {"IVG_INFLIGHT_WARM", "1"}, {"IVG_DG2_MF_CAP", "1"}, {"IVG_INFLIGHT_KB", "40,40,40,40,40"}, {"IVG_INFLIGHT_GEMM256", "0"},
};

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL (line %d): ", __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fputc('\n', stderr); ++g_fail; } } while (0)

static void clear_env() {
  std::vector<std::string> names;
  for (char** p = environ; *p; ++p)
    if (!std::strncmp(*p, "IVG_", 4)) names.emplace_back(*p, std::strcspn(*p, "="));
  for (const std::string& n : names) unsetenv(n.c_str());
}

// every field but `skip` (-1: none) holds its default
static void expect_defaults(const Switches& s, int skip, const char* what) {
  for (int i = 0; i < kDocN; ++i)
    if (i != skip) EXPECT(s.*kDoc[i].field == kDoc[i].dflt, "%s: %s is %d, default %d", what, kDoc[i].env, s.*kDoc[i].field, kDoc[i].dflt);
}

static int field_after(const char* env, const char* raw, int Switches::*field) {
  setenv(env, raw, 1);
  reload_switches();
  const int v = sw().*field;
  unsetenv(env);
  reload_switches();
  return v;
}

int main() {
  clear_env();
  // clean environment: the documented defaults; the first read publishes generation 1
  expect_defaults(sw(), -1, "clean environment");
  const unsigned g0 = switches_generation();
  EXPECT(g0 == 1, "first read: generation %u", g0);
  const Switches* first = &sw();
  reload_switches();
  EXPECT(switches_generation() == g0 && &sw() == first, "a reload with unchanged values published a table");

  // without IVG_DEV=1 (unset, and at a value other than 1) a development variable changes nothing
  for (const char* dev : {(const char*)nullptr, "0", "2"}) {
    if (dev) setenv("IVG_DEV", dev, 1);
    for (int i = 0; i < kDocN; ++i) {
      if (!kDoc[i].dev) continue;
      setenv(kDoc[i].env, kDoc[i].other, 1);
      reload_switches();
      expect_defaults(sw(), -1, kDoc[i].env);
      EXPECT(switches_generation() == g0, "%s without IVG_DEV=1 moved the generation", kDoc[i].env);
      unsetenv(kDoc[i].env);
    }
    unsetenv("IVG_DEV");
  }

  // each variable changes exactly its own field (development ones under IVG_DEV=1), one generation per change
  setenv("IVG_DEV", "1", 1);
  reload_switches();
  EXPECT(switches_generation() == g0, "IVG_DEV=1 alone moved the generation");
  unsigned g = g0;
  for (int i = 0; i < kDocN; ++i) {
    setenv(kDoc[i].env, kDoc[i].other, 1);
    reload_switches();
    EXPECT(sw().*kDoc[i].field == kDoc[i].other_val, "%s=%s gives %d", kDoc[i].env, kDoc[i].other, sw().*kDoc[i].field);
    expect_defaults(sw(), i, kDoc[i].env);
    EXPECT(switches_generation() == g + 1, "%s=%s: generation %u after %u", kDoc[i].env, kDoc[i].other, switches_generation(), g);
    reload_switches();
    EXPECT(switches_generation() == g + 1, "%s: a second reload of the same values moved the generation", kDoc[i].env);
    unsetenv(kDoc[i].env);
    reload_switches();
    expect_defaults(sw(), -1, "variable removed again");
    EXPECT(switches_generation() == g + 2, "%s removed: generation %u after %u", kDoc[i].env, switches_generation(), g + 1);
    g += 2;
  }

  // normalisations (IVG_DEV=1 still set)
  EXPECT(field_after("IVG_DECODE_LDS_KB", "8", &Switches::decode_lds_kb) == 160, "IVG_DECODE_LDS_KB=8");
  EXPECT(field_after("IVG_DECODE_LDS_KB", "999", &Switches::decode_lds_kb) == 160, "IVG_DECODE_LDS_KB=999");
  EXPECT(field_after("IVG_DECODE_LDS_KB", "16", &Switches::decode_lds_kb) == 16, "IVG_DECODE_LDS_KB=16");
  EXPECT(field_after("IVG_DECODE_LDS_KB", "", &Switches::decode_lds_kb) == 160, "IVG_DECODE_LDS_KB empty");
  EXPECT(field_after("IVG_GRAPH", "2", &Switches::graph) == 0, "IVG_GRAPH=2");
  EXPECT(field_after("IVG_CONV_CAP", "2", &Switches::conv_cap) == 0, "IVG_CONV_CAP=2");
  EXPECT(field_after("IVG_CONV_CAP", "1", &Switches::conv_cap) == 1, "IVG_CONV_CAP=1");
  EXPECT(field_after("IVG_CONV3X3", "2", &Switches::conv3x3) == 1, "IVG_CONV3X3=2 is on, stored as 1");
  EXPECT(field_after("IVG_DG3", "", &Switches::dg3) == 1, "IVG_DG3 empty");

  // the retired names are no switches any more
  g = switches_generation();
  for (const auto& r : kRetired) {
    setenv(r[0], r[1], 1);
    reload_switches();
    expect_defaults(sw(), -1, r[0]);
    EXPECT(switches_generation() == g, "retired %s moved the generation", r[0]);
    unsetenv(r[0]);
  }

  if (g_fail) { std::fprintf(stderr, "switches_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("switches_check: %d switches, %d retired names ok\n", kDocN, (int)(sizeof(kRetired) / sizeof(kRetired[0])));
  return 0;
}
