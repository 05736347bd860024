"""Which kernels the no-blank and binary entry points launch, shape by shape.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/kernel_sweep.py      (on the GPU)
    python tools/kernel_sweep.py --reduce OUT > trace.txt                                     (anywhere)

The sweep calls every no-blank and binary entry point once per shape -- loss with gradient (+ backward: scale_grad),
loss without, smoothed loss, bf16 / fp16 loss, posteriors, best path -- over the bench.py workloads (the blank one: its
loss alone), the strong-scaling batch of 2048 and the shape lists of the kernel-path tests of
tests/test_parity_gpu.py.  A call the library refuses launches nothing.  `--reduce` turns the trace into one line per
launch of a `ctc::` kernel, in launch order: kernel name, grid (in threads), workgroup and LDS size.  Two builds select
the same kernels iff their reduced traces are equal line for line (diff them); profiles/r08_kernel_selection.md keeps
the pair taken when the host side of noblank.hip was split into parameters, plan and launch."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOBLANK = [
    (150, 256, 158, 20), (150, 2048, 158, 20),                                                   # bench.py, strong scaling
    (1, 1, 1, 1), (1, 3, 5, 1), (165, 3, 70, 9), (168, 2, 33, 10), (169, 2, 33, 10), (400, 2, 40, 12),   # path boundaries
    (30, 9, 256, 64), (30, 2, 257, 65), (12, 2, 20, 256),
    (168, 3, 256, 31), (150, 2, 158, 20), (9, 2, 2, 5), (40, 2, 34, 17), (33, 4, 64, 16),         # r16 cases
    (20, 4, 10, 5), (150, 8, 158, 20), (40, 3, 300, 70), (168, 5, 64, 31), (61, 300, 34, 9), (50, 6, 33, 12),  # posteriors
    (2000, 2, 50, 20), (700, 3, 300, 40), (900, 2, 20, 100),                                      # workspace lattice
    (150, 700, 158, 20), (60, 530, 64, 31), (37, 600, 34, 9), (90, 1030, 192, 12), (168, 515, 20, 5),   # persistent
    (150, 2100, 158, 20),
]
BINARY = [
    (150, 256, 158, 20), (150, 2048, 158, 20),
    (1, 1, 1, 1), (170, 2, 40, 12), (160, 2, 158, 20), (30, 2, 257, 6), (30, 3, 64, 64), (20, 2, 30, 70),
    (168, 2, 40, 12), (169, 2, 40, 12), (161, 3, 158, 20), (29, 2, 256, 64), (3, 2, 20, 3), (28, 3, 63, 63),
    (15, 2, 130, 17), (57, 2, 129, 33),
    (20, 4, 10, 5), (150, 8, 158, 20), (37, 5, 64, 7), (60, 2, 40, 64), (168, 3, 33, 10),
]


def sweep():
    import torch
    import ctc_amd
    from tests.helpers import synth_binary, synth_blank, synth_noblank
    dev = torch.device("cuda:0")

    def call(what, shape, fn):
        try:
            fn()
            print("%-28s %s" % (what, shape), flush=True)
        except ctc_amd.CtcAmdError as e:
            print("%-28s %s refused: %s" % (what, shape, str(e)[:60]), flush=True)
        torch.cuda.synchronize()

    def loss_backward(fn, x, *rest, **kw):
        x = x.detach().requires_grad_(True)
        fn(x, *rest, **kw)[0].backward()

    for shape in NOBLANK:
        T, B, C, S = shape
        x, lab, Tb, L = (t.to(dev) for t in synth_noblank(sum(shape), T, B, C, S, var_T=T > 4))
        L = torch.minimum(L, Tb)
        call("noblank loss+grad", shape, lambda: loss_backward(ctc_amd.noblank_ctc_loss, x, lab, Tb, L))
        call("noblank loss", shape, lambda: ctc_amd.noblank_ctc_loss(x, lab, Tb, L))
        call("noblank smoothed loss+grad", shape,
             lambda: loss_backward(ctc_amd.noblank_ctc_loss, x, lab, Tb, L, label_smoothing=0.9))
        for dt in (torch.bfloat16, torch.float16):
            xl = x.to(dt)
            call("noblank %s loss+grad" % str(dt)[6:], shape, lambda: loss_backward(ctc_amd.noblank_ctc_loss, xl, lab, Tb, L))
        call("noblank posteriors", shape, lambda: ctc_amd.noblank_posteriors(x, lab, Tb, L))
        call("noblank best path", shape, lambda: ctc_amd.noblank_best_path(x, lab, Tb, L))
    for shape in BINARY:
        T, B, C, S = shape
        x, y, Tb, L = (t.to(dev) for t in synth_binary(sum(shape), T, B, C, S, var_T=T > 4, density=0.2))
        L = torch.minimum(L, Tb)
        call("binary loss+grad", shape, lambda: loss_backward(ctc_amd.binary_ctc_loss, x, y, Tb, L))
        call("binary loss", shape, lambda: ctc_amd.binary_ctc_loss(x, y, Tb, L))
        call("binary posteriors", shape, lambda: ctc_amd.binary_posteriors(x, y, Tb, L))
        call("binary best path", shape, lambda: ctc_amd.binary_best_path(x, y, Tb, L))
    shape = (2000, 64, 1000, 100)                            # bench.py's third workload (its kernels are not touched)
    x, tg, Tb, L = (t.to(dev) for t in synth_blank(0, *shape))
    call("blank loss+grad", shape, lambda: loss_backward(ctc_amd.blank_ctc_loss, x, tg, Tb, L))


def reduce(out):
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    col = lambda r, prefix: "x".join(r[k] for k in sorted(r) if k.startswith(prefix))
    print("# kernel | grid | workgroup | LDS bytes")
    for r in rows:
        if "ctc::" in r["Kernel_Name"] or "_ZN3ctc" in r["Kernel_Name"]:     # (the profiler leaves __bf16 instantiations mangled)
            print("%s | %s | %s | %s" % (r["Kernel_Name"], col(r, "Grid_Size"), col(r, "Workgroup_Size"), col(r, "LDS")))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    else:
        sweep()
