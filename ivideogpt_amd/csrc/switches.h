// Every run-time switch of libivg, in ONE place.  The table is read from the environment when the library is loaded, again at
// every ivg_create and on ivg_reload_switches() (tests flip a variable, then call it); the kernels' launchers only ever read the
// published table -- no getenv() and no lazily initialised static on a launch path, so engines driven from several host threads
// (bench.py --lanes, replica()) share nothing that is written after start-up.
//
// Two classes (round 6: the settled A/B switches left the product surface):
//   * LAUNCH POLICY -- honoured always: how a deployment wants the same kernels launched.
//   * DEVELOPMENT -- honoured only when IVG_DEV=1 is set in the environment as well: which of two kernels runs a shape.  They exist
//     so that a test can put the alternative path (the one the fp32 parity mode or an uncovered shape takes anyway) beside the default
//     on the same inputs; without IVG_DEV=1 a stray variable changes nothing.  tests/conftest.py's `switches` fixture sets it.
//
//   variable                 default  meaning
//   ---- launch policy
//   IVG_GRAPH                0        1: decode steps replayed from hipGraphs (8 steps per launch) instead of eager launches
//   IVG_DECODE_LDS_KB        160      process-wide default of ivg_config.decode_lds_kb: LDS budget of a decode-GEMM workgroup in KiB; a
//                                        budget below 160 is the batches-in-flight profile (see include/ivg.h)
//   ---- development (IVG_DEV=1)
//   IVG_CONV3X3              1        0: every 3x3 convolution on the generic implicit GEMM (igemm.hip)
//   IVG_SUBPIXEL             1        0: nearest-x2 upsampling convolutions as nine taps over the upsampled grid (1: four 2x2 phase
//                                        convolutions over the low-resolution input with pre-summed weights, conv3x3.hip SUBPIX)
//   IVG_GEMM256              1        0: large dense GEMMs on the generic implicit GEMM
//   IVG_KV24                 1        0: the x3 rollout keeps an fp32 K / V cache (1: 24 bits per element in two planes, llama_ops.hip)
//   IVG_GEMM256X3            1        0: large dense split-bf16 ("x3") GEMMs on the generic implicit GEMM's X3 instance (1: 256 x 256 tiles)
//   IVG_DG3                  1        0: decode GEMMs on the second-generation kernel (dgemm.hip)
//   IVG_FLASH_PREFILL        1        0: prompt attention as score GEMM + softmax + P.V GEMM (what the fp32 engine mode runs)
//   IVG_KV_EXTEND_CHUNK      1        0: ivg_kv_extend appends by decode steps with given inputs on every engine (1: one chunk pass over the
//                                        given tokens where the cache is native bf16 at head_dim 64, transformer.cpp Run::extend)
//   IVG_GN_APPLY_FUSE        1        0: GroupNorm + SiLU as a separate apply pass (1: inside the consuming conv3x3's halo staging)
//   IVG_X3                   1        0: the fp32 decode path of the tokenizer on f32-input MFMAs (1: split-bf16 "x3" convolutions)
//   IVG_CONV_CAP             0        1: conv3x3 grids at ONE workgroup per CU (LDS padded past half a CU's 160 KiB)
//   IVG_DECODE_ATTN_WINDOW   1        0: bf16 head_dim-64 decode attention on the two-buffer body (1: one row buffer as a rolling window, half the
//                                        registers; bit-identical outputs -- llama_ops.hip decode_attn_kernel WINDOW)
#pragma once

namespace ivg {

// A new switch is a field here, a row of the table in switches.cpp (name, default, class, normalisation) and a line above.
struct Switches {
  int graph, decode_lds_kb;
  int conv3x3, subpixel, gemm256, gemm256x3, kv24, dg3, flash_prefill, kv_extend_chunk, gn_apply_fuse, x3, conv_cap, decode_attn_window;
  bool operator==(const Switches& o) const;   // over the rows of the table
};

const Switches& sw();             // the published table: immutable, never freed or rewritten (a reload that changes it publishes a NEW one)
void reload_switches();           // re-read the environment; publishes a new table (and a new generation) only when a field changed
unsigned switches_generation();   // incremented by every reload that changed the table (part of the key of captured step graphs)

}  // namespace ivg
