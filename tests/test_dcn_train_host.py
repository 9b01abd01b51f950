"""Host surface of DCN head training (no GPU): the new entry points are declared, the autograd function exists, and on CPU tensors
DCNSepHead in .train() still runs the torch restatement."""
import copy
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_deform_adapt_backward_workspace_bytes", "fd_deform_adapt_backward", "fd_deform_adapt_pack_weight_device")


def test_new_entry_points_are_declared_with_matching_arity():
    from futuredet_amd import lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "futuredet_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert name in lib.SIGNATURES, name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, "%s is not declared in futuredet_hip.h" % name
        params = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(params) == len(lib.SIGNATURES[name][1]), (name, len(params), len(lib.SIGNATURES[name][1]))
    assert lib.ABI_VERSION == 8


def test_the_source_is_built_with_the_forward_flags():
    from futuredet_amd import build

    assert "fd_deform_conv_grad.hip" in build.SOURCES
    assert build.EXTRA["fd_deform_conv_grad.hip"] == build.EXTRA["fd_deform_conv.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]


def test_the_autograd_function_and_front_end_exist():
    from futuredet_amd import heads, hip_ops

    assert issubclass(heads._DeformAdaptFunction, torch.autograd.Function)
    assert callable(hip_ops.deform_adapt_backward) and callable(hip_ops.pack_deform_adapt_device)


def test_cpu_training_still_runs_the_restatement():
    from futuredet_amd.heads import DCNSepHead

    torch.manual_seed(3)
    head = DCNSepHead(64, 1, dict(reg=(2, 2), height=(1, 2)), bn=True, final_kernel=3).train()
    for fa in (head.feature_adapt_cls, head.feature_adapt_reg):
        fa.conv_offset.weight.data.normal_(0, 0.05)
        fa.conv_offset.bias.data.uniform_(-1, 1)
    ref = copy.deepcopy(head)
    x = torch.relu(torch.randn(1, 64, 7, 6))
    seen = {}
    hooks = [head.cls_head.register_forward_pre_hook(lambda m, a: seen.__setitem__("cls", a[0])),
             head.task_head.register_forward_pre_hook(lambda m, a: seen.__setitem__("reg", a[0]))]
    xa = x.clone().requires_grad_(True)
    out = head(xa)
    for h in hooks:
        h.remove()
    xb = x.clone().requires_grad_(True)
    rc, rr = ref.feature_adapt_cls(xb), ref.feature_adapt_reg(xb)
    assert torch.equal(seen["cls"], rc) and torch.equal(seen["reg"], rr)
    want = ref.task_head(rr)
    want["hm"] = ref.cls_head(rc)
    assert set(out) == set(want)
    for k in out:
        assert torch.equal(out[k], want[k]), k
    sum(v.sum() for v in out.values()).backward()
    sum(v.sum() for v in want.values()).backward()
    assert torch.equal(xa.grad, xb.grad)
    for (n, p), (_, q) in zip(head.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), n
