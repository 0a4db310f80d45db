"""Launch the rollout's sampler kernel on bench-shaped logits (run under rocprofv3 --kernel-trace to time it).

    python tools/sampler_bench.py [V]                       launches: the plain sampler, then the nucleus arms
    python tools/sampler_bench.py --summarize TRACE.csv [V]  µs per launch of each nucleus arm from the kernel trace of that run

Nucleus arms (ivg_op_sample_top_p, B = 64): k=100/p=1 (the plain kernel), k=100/p=0.9 (list path), k=all/p=0.9 (full-vocabulary
path).  Each arm runs WARM untimed launches first (the first launch of an instance sets it up), then TIMED launches; the two p=0.9
arms share a kernel name, so the trace is split by launch order, which is fixed here."""
import ctypes as C
import sys

WARM, TIMED = 10, 40


def arms(V):
    return [("k=100/p=1", 100, 1.0), ("k=100/p=0.9", 100, 0.9), ("k=all/p=0.9", V, 0.9)]


def summarize(path, V):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "sample_embed_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    names = [r["Kernel_Name"] for r in rows]
    per = WARM + TIMED
    us, names = us[-per * len(arms(V)):], names[-per * len(arms(V)):]
    for i, (name, _, _) in enumerate(arms(V)):
        t = sorted(us[i * per + WARM:(i + 1) * per])
        print(f"{name:12s} median {t[len(t) // 2]:7.2f} us  min {t[0]:7.2f}  max {t[-1]:7.2f}  ({TIMED} launches after {WARM} warm-up; "
              f"{names[i * per + WARM].split('(')[0]})")


def main():
    import torch
    from ivideogpt_amd import _lib
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 16386
    l = _lib.load()
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn(64, V, generator=g) * 3).cuda()
    u = torch.rand(64, generator=g).cuda()
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in (100, 100, 100, 100, 1000, 1000):
        assert l.ivg_op_sample(C.c_void_p(lg.data_ptr()), 64, V, k, 1.0, C.c_void_p(u.data_ptr()), C.c_void_p(out.data_ptr()), st) == 0
    for _ in range(3):
        assert l.ivg_op_sample(C.c_void_p(lg.data_ptr()), 64, V, 100, 1.0, None, C.c_void_p(out.data_ptr()), st) == 0
    for _, k, p in arms(V):
        for _ in range(WARM + TIMED):
            assert l.ivg_op_sample_top_p(C.c_void_p(lg.data_ptr()), 64, V, k, 1.0, p, C.c_void_p(u.data_ptr()), C.c_void_p(out.data_ptr()),
                                         st) == 0
    torch.cuda.synchronize()
    print("ok", out[:4].tolist())


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 16386)
    else:
        main()
