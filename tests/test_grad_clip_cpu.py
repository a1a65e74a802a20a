"""The gradient-clip entries (dppo_grad_clip_workspace_bytes, dppo_grad_clip_scales,
dppo_optimizer_step_clip) as far as they go without a GPU: they are declared, bound and exported, the
workspace query is host arithmetic, and every refusal comes back with its code and message before
anything touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dppo.h")
NEW = ("dppo_grad_clip_workspace_bytes", "dppo_grad_clip_scales", "dppo_optimizer_step_clip")


@pytest.fixture(scope="module")
def lib():
    from diffusionpolicyoptimization_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "diffusionpolicyoptimization_amd", "csrc"), "-j8"],
                       check=True)
    return _lib.load()


def test_clip_symbols_declared_bound_and_exported(lib):
    from diffusionpolicyoptimization_amd import _lib
    src = open(HEADER).read()
    declared = set(re.findall(r"DPPO_API\s+[\w\s\*]+?\b(dppo_\w+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dppo_\w+)", nm))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in exported, name
    assert lib.dppo_abi_version() == 15          # additions within ABI 15
    assert (_lib.DPPO_NET_ACTOR, _lib.DPPO_NET_CRITIC) == (1, 2)
    assert re.search(r"DPPO_NET_ACTOR\s*=\s*1\s*,\s*DPPO_NET_CRITIC\s*=\s*2", src)


def test_clip_workspace_bytes_host_arithmetic(lib):
    """One fp64 partial per chunk: nonzero for each network, and monotone in the set of networks
    (both >= either alone; the two ranges' chunks add up, since no chunk crosses a variable)."""
    from diffusionpolicyoptimization_amd import ops
    for d in (ops.ModelDims(), ops.ModelDims(obs_dim=17, action_dim=6), ops.ModelDims(action_dim=3, horizon_steps=3)):
        c = d.c()
        a, k, both = (lib.dppo_grad_clip_workspace_bytes(ctypes.byref(c), n) for n in (1, 2, 3))
        assert a > 0 and k > 0 and a % 8 == 0 and k % 8 == 0
        assert both >= a and both >= k and both == a + k
        assert 8 * 12 <= a and 8 * 8 <= k          # at least one chunk per variable
        assert ops.grad_clip_workspace_bytes(d, "both") == both
        for bad in (0, 4, -1):
            assert lib.dppo_grad_clip_workspace_bytes(ctypes.byref(c), bad) == 0
    bad_dims = ops.ModelDims(actor_hidden=100).c()
    assert lib.dppo_grad_clip_workspace_bytes(ctypes.byref(bad_dims), 1) == 0


def test_grad_clip_scales_refusals_need_no_device(lib):
    from diffusionpolicyoptimization_amd import ops
    c = ops.ModelDims().c()
    buf = (ctypes.c_double * 64)()            # never dereferenced: every call below is refused first
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.dppo_last_error().decode()
    for nets in (0, 4, -2):
        assert lib.dppo_grad_clip_scales(ctypes.byref(c), nets, p, 1.0, None, p, p, None) == 1
        assert "nets" in err()
    for clip in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dppo_grad_clip_scales(ctypes.byref(c), 3, p, clip, None, p, p, None) == 1
        assert "clip_norm" in err()
    assert lib.dppo_grad_clip_scales(ctypes.byref(c), 1, None, 1.0, None, p, p, None) == 1 and "NULL" in err()
    assert lib.dppo_grad_clip_scales(ctypes.byref(c), 1, p, 1.0, None, None, p, None) == 1 and "NULL" in err()
    assert lib.dppo_grad_clip_scales(ctypes.byref(c), 1, p, 1.0, None, p, None, None) == 1 and "workspace" in err()
    bad = ops.ModelDims(time_dim=3).c()
    assert lib.dppo_grad_clip_scales(ctypes.byref(bad), 1, p, 1.0, None, p, p, None) == 1 and "time_dim" in err()
    assert lib.dppo_grad_clip_scales(None, 1, p, 1.0, None, p, p, None) == 1


def test_optimizer_step_clip_refusals_need_no_device(lib):
    from diffusionpolicyoptimization_amd import _lib, ops
    d = ops.ModelDims()
    c = d.c()
    na, nc = ops.spec_count(ops.actor_param_spec(d)), ops.spec_count(ops.critic_param_spec(d))
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.dppo_last_error().decode()

    def step(n, mode, scales, nets, prec=0):
        return lib.dppo_optimizer_step_clip(ctypes.byref(c), prec, p, p, p, p, n, 1, 1e-3, 0.004, 0.9, 0.999, 1e-7, mode,
                                            None, None, None, None, None, None, 0, 0, None, None, 0, None, scales, nets)
    for nets in (0, 4):
        assert step(na, 0, p, nets) == 1 and "nets" in err()
    assert step(na, 0, None, 1) == 1 and "clip_scales" in err()
    assert step(na, _lib.DPPO_STEP_L2_FROM_PL2, p, 1) == 1 and "DPPO_STEP_L2_FROM_PL2" in err()
    # the range must be the whole network(s) nets names
    for n, nets in ((na - 1, 1), (nc, 1), (na, 2), (na + nc - 4, 3), (na, 3)):
        assert step(n, 0, p, nets) == 1 and "exactly" in err(), (n, nets)
    assert step(na, 0, p, 1, prec=7) == 1 and "precision" in err()


def test_python_wrappers_validate_before_the_library():
    """ops.BoundGradClip / BoundOptimizerStep reject what they can see on the host."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d = ops.ModelDims()
    g = torch.zeros(10)
    with pytest.raises(ValueError, match="nets"):
        ops.BoundGradClip(d, 5, g, 1.0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.BoundGradClip(d, "actor", g, 1.0)
