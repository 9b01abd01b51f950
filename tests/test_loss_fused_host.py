"""The host side of the fused CenterHead loss (csrc/fd_loss.hip): exported symbols, struct mirrors, the argument checks of both entry
points (no device needed: they validate before any device work), the skip-and-count guard through a stand-alone program, and the
``fused_loss`` switch on CPU tensors.  CPU only."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_loss as mgl  # noqa: E402
from futuredet_amd import build, build_head, hip_ops, lib  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "loss.npz"))
NAMES = {"fd_loss_chunk", "fd_centerhead_loss_terms", "fd_centerhead_loss_workspace_bytes", "fd_centerhead_loss_forward",
         "fd_centerhead_loss_backward"}


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def _cfg(**kw):
    args = dict(B=4, H=180, W=180, M=1000, n_tasks=1, dense=False, T=7, D=10, row_stride=10, code_weights=[1.0] * 10,
                code_weights_forecast=[0.5] * 10, weight=0.25)
    args.update(kw)
    return hip_ops.make_loss_cfg(**args)


def test_symbols_build_flags_and_chunk(L):
    assert NAMES <= set(lib.SIGNATURES)
    assert "fd_loss.hip" in build.SOURCES and build.EXTRA["fd_loss.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION
    assert L.fd_loss_chunk() > 0 and L.fd_loss_chunk() == int(re.search(r"#define FD_LOSS_CHUNK (\d+)", hdr).group(1)) == hip_ops.loss_chunk()


def test_struct_mirrors(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "futuredet_hip.h")).read(), flags=re.S)
    pairs = {"fd_loss_cfg": lib.LossCfg, "fd_loss_task": lib.LossTask}
    for cname, mirror in pairs.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, flags=re.S).group(1)
        members = []
        for decl in body.split(";"):
            m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[(\d+)\])?\s*$", decl.strip())
            if decl.strip():
                members.append((m.group(1), int(m.group(3)) if m.group(3) else None))
        assert [(n, getattr(t, "_length_", None)) for n, t in mirror._fields_] == members, cname
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "futuredet_hip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(fd_loss_cfg), sizeof(fd_loss_task)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [ctypes.sizeof(lib.LossCfg), ctypes.sizeof(lib.LossTask)]


def test_workspace_and_terms_sizes(L):
    ws = [L.fd_centerhead_loss_workspace_bytes(ctypes.byref(_cfg(n_tasks=n)), 1) for n in (1, 2, 7, 16)]
    assert 0 < ws[0] < ws[1] < ws[2] < ws[3]
    assert L.fd_centerhead_loss_workspace_bytes(ctypes.byref(_cfg()), 3) > ws[0]
    assert L.fd_centerhead_loss_terms(ctypes.byref(_cfg())) == 1 * (4 + 7 + 70) + 1
    assert L.fd_centerhead_loss_terms(ctypes.byref(_cfg(dense=True, n_tasks=7))) == 7 * (4 + 1 + 10) + 1
    assert hip_ops.loss_terms_layout(_cfg()) == (81, 7) and hip_ops.loss_terms_layout(_cfg(dense=True)) == (15, 1)
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(M=0), dict(n_tasks=0), dict(n_tasks=17), dict(T=0), dict(T=8), dict(M=4096)):
        assert L.fd_centerhead_loss_workspace_bytes(ctypes.byref(_cfg(**bad)), 1) == 0, bad
        assert L.fd_centerhead_loss_terms(ctypes.byref(_cfg(**bad))) == 0, bad
    c = _cfg()
    c.D = 9
    assert L.fd_centerhead_loss_workspace_bytes(ctypes.byref(c), 1) == 0
    assert L.fd_centerhead_loss_workspace_bytes(ctypes.byref(_cfg()), 0) == 0 and L.fd_centerhead_loss_workspace_bytes(None, 1) == 0
    assert L.fd_centerhead_loss_workspace_bytes(ctypes.byref(_cfg(dense=True, T=99, n_tasks=7)), 1) > 0  # a dense head ignores T
    assert hip_ops.loss_columns(14, 14) == list(range(14)) and hip_ops.loss_columns(10, 14) == [0, 1, 2, 3, 4, 5, 6, 7, 12, 13]
    assert hip_ops.loss_columns(8, 10) == [0, 1, 2, 3, 4, 5, 8, 9]
    with pytest.raises(ValueError):
        hip_ops.make_loss_cfg(1, 8, 8, 4, 1, False, 1, 10, 10, [1.0] * 8)


def _tasks(n, fill=0x1000, C=1):
    """n descriptors whose pointers are never dereferenced: the calls below fail validation before any device work"""
    arr = (lib.LossTask * n)()
    for t in arr:
        t.hm = t.hm_target = t.ind = t.cat = t.sig = t.d_hm = fill
        for i in range(7):
            t.mask[i] = t.maps[i] = t.anno_box[i] = t.d_maps[i] = fill
        t.C = C
    return arr


def test_invalid_arguments_are_einval_without_a_device(L):
    ok = _cfg()
    ws = ctypes.c_void_p(0x10000)
    big = 1 << 40
    terms = go = ctypes.c_void_p(0x2000)

    def both(cfg, tasks, text, ws=ws, ws_bytes=big):
        for rc in (L.fd_centerhead_loss_forward(cfg, tasks, terms, ws, ws_bytes, None),
                   L.fd_centerhead_loss_backward(cfg, tasks, terms, go, ws, ws_bytes, None)):
            assert rc == -1 and text in L.fd_last_error().decode(), (text, L.fd_last_error())

    both(None, _tasks(1), "null cfg")
    both(ctypes.byref(ok), None, "null tasks")
    both(ctypes.byref(ok), _tasks(1), "null workspace", ws=None)
    for bad, text in ((dict(B=0), "must be positive"), (dict(H=-3), "must be positive"), (dict(W=0), "must be positive"), (dict(M=0), "must be positive"),
                      (dict(n_tasks=17), "n_tasks (17)"), (dict(n_tasks=0), "n_tasks (0)"), (dict(T=0), "T (0)"), (dict(T=8), "T (8)"),
                      (dict(M=4096), "objects per sample")):
        both(ctypes.byref(_cfg(**bad)), _tasks(max(1, min(bad.get("n_tasks", 1), 17))), text)
    c = _cfg()
    c.D = 12
    both(ctypes.byref(c), _tasks(1), "D (12)")
    c = _cfg()
    c.col[9] = 10
    both(ctypes.byref(c), _tasks(1), "outside a target row")
    both(ctypes.byref(ok), _tasks(1, C=0), "C (0)")
    both(ctypes.byref(_cfg(B=128, H=1440, W=1440)), _tasks(1), "2^31")
    need = L.fd_centerhead_loss_workspace_bytes(ctypes.byref(ok), 1)
    both(ctypes.byref(ok), _tasks(1), "workspace too small", ws_bytes=need - 1)
    t = _tasks(1)
    t[0].cat = None
    both(ctypes.byref(ok), t, "null hm, hm_target, ind or cat")
    t = _tasks(1)
    t[0].anno_box[6] = None
    both(ctypes.byref(ok), t, "null mask or anno_box of step 6")
    t = _tasks(1)
    t[0].maps[3] = None
    both(ctypes.byref(ok), t, "null map 3")
    t = _tasks(1)
    t[0].maps[4] = None  # rvel: not part of a 10-channel head, may be null
    t[0].sig = None
    assert L.fd_centerhead_loss_forward(ctypes.byref(ok), t, terms, ws, big, None) == -1 and "null sig" in L.fd_last_error().decode()
    assert L.fd_centerhead_loss_forward(ctypes.byref(ok), _tasks(1), None, ws, big, None) == -1 and "null terms" in L.fd_last_error().decode()
    assert L.fd_centerhead_loss_backward(ctypes.byref(ok), _tasks(1), terms, None, ws, big, None) == -1 and "null terms or go" in L.fd_last_error().decode()


GUARD_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "fd_loss_guard.h"
// reads "mask ind cat" triples; gathers the taken ones from a [B, C, HW] map that is allocated exactly (a sanitizer sees any
// index past it) and prints what the kernels accumulate: entries taken, entries counted in the status word, the gathered sum
int main(int argc, char **argv) {
    const int B = atoi(argv[1]), C = atoi(argv[2]);
    const long long hw = atoll(argv[3]);
    float *map = (float *)malloc(sizeof(float) * B * C * hw);
    for (long long i = 0; i < B * C * hw; ++i) map[i] = (float)(i % 251);
    long long take = 0, bad = 0, skip = 0, mask, ind, cat;
    double sum = 0.0;
    int b = 0;
    while (scanf("%lld %lld %lld", &mask, &ind, &cat) == 3) {
        const int kind = fd_loss_entry_kind((uint8_t)mask, ind, cat, hw, C);
        if (kind == kLossSkip) { ++skip; }
        else if (kind == kLossBad) { ++bad; }
        else {
            const int64_t e = fd_loss_cell(b, B, (int)cat, C, ind, hw);
            if (e < 0) return 3;
            sum += map[e];
            ++take;
        }
        b = (b + 1) % B;
    }
    if (fd_loss_cell(B, B, 0, C, 0, hw) != -1 || fd_loss_cell(0, B, C, C, 0, hw) != -1 || fd_loss_cell(0, B, 0, C, hw, hw) != -1 ||
        fd_loss_cell(-1, B, 0, C, 0, hw) != -1 || fd_loss_cell(0, B, -1, C, 0, hw) != -1 || fd_loss_cell(0, B, 0, C, -1, hw) != -1) return 4;
    printf("%lld %lld %lld %.1f\n", take, bad, skip, sum);
    free(map);
    return 0;
}
"""


def test_skip_and_count_guard_through_a_stand_alone_program(tmp_path):
    """csrc/fd_loss_guard.h is what the kernels call in front of every gather: mask == 0 is dropped whatever ind / cat hold, a masked
    entry out of range is counted and never turned into an index."""
    src = tmp_path / "guard.cc"
    src.write_text(GUARD_MAIN)
    exe = str(tmp_path / "guard")
    subprocess.check_call(["g++", "-O1", "-g", "-I", os.path.join(REPO, "futuredet_amd", "csrc"), "-o", exe, str(src)])
    B, C, hw = 3, 2, 35
    rng = np.random.default_rng(0)
    edge = np.array([-(2 ** 62), -(2 ** 31) - 1, -1, 0, 1, hw - 1, hw, hw + 1, 2 ** 31, 2 ** 32 + 3, 2 ** 62])
    rows = [(int(m), int(i), int(c)) for m in (0, 1, 255) for i in edge for c in (-(2 ** 40), -1, 0, 1, C, 2 ** 33)]
    rows += [(int(m), int(i), int(c)) for m, i, c in zip(rng.integers(0, 2, 400), rng.integers(-5, hw + 5, 400), rng.integers(-1, C + 1, 400))]
    take = bad = skip = 0
    total = 0.0
    for n, (m, i, c) in enumerate(rows):
        if m == 0:
            skip += 1
        elif 0 <= i < hw and 0 <= c < C:
            take += 1
            total += float((((n % B) * C + c) * hw + i) % 251)
        else:
            bad += 1
    out = subprocess.run([exe, str(B), str(C), str(hw)], input="".join("%d %d %d\n" % r for r in rows).encode(), stdout=subprocess.PIPE, check=True).stdout
    assert out.decode().split() == [str(take), str(bad), str(skip), "%.1f" % total]
    assert take > 50 and bad > 100 and skip > 100


def test_fused_loss_defaults_to_false_and_is_no_constructor_argument():
    head = build_head(dict(type="CenterHead", **mgl.head_kwargs(1, False)))
    assert head.fused_loss is False
    with pytest.raises(TypeError):
        build_head(dict(type="CenterHead", fused_loss=True, **mgl.head_kwargs(1, False)))


@pytest.mark.parametrize("name,T,dense", mgl.CASES)
def test_switch_on_keeps_the_torch_path_for_cpu_double_maps(name, T, dense):
    head = build_head(dict(type="CenterHead", **mgl.head_kwargs(T, dense))).double()
    head.fused_loss = True
    d = {k: GOLD[k] for k in GOLD.files}
    ret, grads = mgl.run_loss(head, d, name, T, dense)
    for k, v in mgl.flatten(ret, name, T, dense).items():
        np.testing.assert_allclose(v, GOLD[k], rtol=1e-10, atol=1e-12, err_msg=k)
    for k, g in grads.items():
        np.testing.assert_allclose(g, GOLD["%s_grad_%s" % (name, k[len(name) + 1:])], rtol=1e-10, atol=1e-12, err_msg=k)


def test_other_modes_still_raise_with_the_switch_on():
    for flag in ("reverse", "sparse", "wide_head", "classify"):
        head = build_head(dict(type="CenterHead", **dict(mgl.head_kwargs(3, False), **{flag: True})))
        head.fused_loss = True
        with pytest.raises(NotImplementedError, match=flag):
            head.loss({}, [])
