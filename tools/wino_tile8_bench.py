"""Winograd tiles 6 / 7 / 8 of fd_conv2d_wino_nhwc_f32 on the flagship layer shapes at B = 2, graph-timed (20 launches per graph,
median of 5 replays; us per launch).  usage: python tools/wino_tile8_bench.py  (with FD_LIB_PATH=<tuning build>: tiles 7 and 8 only)"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from futuredet_amd import hip_ops
def timeit(fn, iters=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters): fn()
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1) / iters)
    return sorted(ts)[2]
for cin, cout, hw in [(256,128,180),(128,128,180),(256,256,90),(512,64,180),(64,384,180)]:
    x = torch.randn(2, hw, hw, cin, device="cuda"); w = torch.randn(cout, cin, 3, 3) * 0.02; b = torch.randn(cout, device="cuda")
    wp = hip_ops.pack_conv2d_weight_wino(w).cuda(); out = torch.empty(2, hw, hw, cout, device="cuda")
    line = "B=2 %d->%d@%d" % (cin, cout, hw)
    r = {}
    for t in ((6, 7, 8) if not os.environ.get("FD_LIB_PATH") else (7, 8)):
        r[t] = timeit(lambda: hip_ops.conv2d_wino_nhwc_f32(x, wp, b, cout, True, out=out, tile=t))
        line += " | tile%d %.1f us" % (t, r[t])
    line += " | tile8/tile7 %.3f" % (r[8] / r[7])
    print(line, flush=True)
