"""train.max_grad_norm on the device: the per-variable norm / clip-scale kernel (dppo_grad_clip_scales)
against NumPy float64, the optimizer steps that apply the scales (dppo_optimizer_step_clip) against
scale-then-step bit for bit, and the agent's clipped split update against the unsplit path, whose clip
is the per-variable torch statement of the reference's tf.clip_by_norm branch
(agent/finetune/train_ppo_diffusion_agent.py:349-354)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = {
    "hopper": {},
    "walker": dict(obs_dim=17, action_dim=6),
    # out_b is 9 elements long: the critic range of [actor | critic] starts on an odd offset, and most
    # variables start off a 16-byte boundary (heads and tails in every chunk)
    "odd": dict(action_dim=3, horizon_steps=3),
}


def _var_sizes(d, nets):
    from diffusionpolicyoptimization_amd import ops
    sizes = []
    if nets & 1:
        sizes += [int(np.prod(s)) for _, s in ops.actor_param_spec(d)]
    if nets & 2:
        sizes += [int(np.prod(s)) for _, s in ops.critic_param_spec(d)]
    return sizes


def _norms64(g, sizes):
    o, out = 0, []
    for k in sizes:
        x = g[o:o + k].astype(np.float64)
        out.append(np.sqrt(np.sum(x * x)))
        o += k
    return np.array(out)


def _gradients(d, nets, seed, clip=1.0):
    """randn * s_v with the per-variable norms spread around the threshold, plus the special variables:
    all zeros, a norm within 1e-3 of the threshold on each side, and entries near 1e20."""
    rng = np.random.default_rng(seed)
    sizes = _var_sizes(d, nets)
    targets = [0.3, 3.0, 0.6, 1.7, 0.05, 25.0, 0.9, 1.2]
    parts = [(rng.standard_normal(k) * (targets[(v + seed) % 8] * clip / np.sqrt(k))).astype(np.float32)
             for v, k in enumerate(sizes)]
    big = int(np.argmax(sizes))                      # l1_w: many chunks
    zero, near_lo, huge = 1, 3, (big + 2) % len(sizes)
    near_hi = big
    parts[zero][:] = 0
    parts[huge] = (rng.standard_normal(sizes[huge]) * 1e20).astype(np.float32)
    for v, f in ((near_hi, 1 + 5e-4), (near_lo, 1 - 5e-4)):
        x = rng.standard_normal(sizes[v])
        parts[v] = (x * (f * clip / np.sqrt(np.sum(x * x)))).astype(np.float32)
    g = np.concatenate(parts)
    ref = _norms64(g, sizes)
    assert ref[zero] == 0 and 0 < ref[near_hi] - clip < 1e-3 * clip and 0 < clip - ref[near_lo] < 1e-3 * clip
    assert ref[huge] > 1e20 and len({zero, near_lo, near_hi, huge}) == 4
    nv = len(sizes)
    assert 3 * int((ref > clip).sum()) >= nv and 3 * int((ref < clip).sum()) >= nv, ref
    return g, sizes, ref


def _check_tables(norms, scales, ref, clip):
    """norms to 2 ulp of fp32 (what fp64 accumulation leaves: the sqrt and the cast); scales exactly 1
    below the threshold by more than that, within 2 ulp of clip / norm elsewhere."""
    norms, scales = norms.astype(np.float64), scales.astype(np.float64)
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    err = np.abs(norms - ref)
    assert np.all(err <= 2 * ulp), (err / ulp).max()
    below = ref < clip - 2 * ulp
    assert np.all(scales[below] == 1.0), scales[below]
    want = clip / ref[~below]
    serr = np.abs(scales[~below] - want)
    assert np.all(serr <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64)), (serr, want)
    assert np.all(np.isfinite(scales)) and np.all(scales <= 1.0) and np.all(scales >= 0.0)


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_norms_and_scales_match_float64(cuda, geometry):
    """dppo_grad_clip_scales for nets = 1, 2, 3 on hopper, walker and a geometry whose variable offsets
    are not multiples of four floats; a second launch on the same input gives identical bits. The
    critic's one-element out_b is the last variable of nets = 2 and 3."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d = ops.ModelDims(**GEOMETRIES[geometry])
    for nets in (1, 2, 3):
        g, sizes, ref = _gradients(d, nets, seed=nets)
        assert nets == 1 or sizes[-1] == 1
        G = torch.tensor(g, device=cuda)
        if geometry == "odd":     # the range itself off a 16-byte boundary: a head in every chunk
            G = torch.cat([G.new_zeros(1), G])[1:]
            assert G.data_ptr() % 16 == 4
        clip = ops.BoundGradClip(d, nets, G, 1.0)
        clip()
        torch.cuda.synchronize()
        n1, s1 = clip.norms.clone(), clip.scales.clone()
        print(geometry, nets, "max norm error in ulp",
              float((np.abs(n1.cpu().numpy().astype(np.float64) - ref) / np.spacing(ref.astype(np.float32))).max()))
        _check_tables(n1.cpu().numpy(), s1.cpu().numpy(), ref, 1.0)
        clip.norms.zero_()
        clip.scales.zero_()
        clip()
        torch.cuda.synchronize()
        assert torch.equal(clip.norms, n1) and torch.equal(clip.scales, s1)
        # the unbound form, without a norm table, and another threshold
        _, s2 = ops.grad_clip_scales(d, nets, G, 0.5, norms=False)
        torch.cuda.synchronize()
        below = ref < 0.5 * (1 - 1e-6)
        assert np.all(s2.cpu().numpy()[below] == 1.0)
        np.testing.assert_allclose(s2.cpu().numpy()[~below], 0.5 / ref[~below], rtol=3e-7)


def test_ticket_is_reusable_across_launches_and_streams(cuda):
    """Three norm launches in a row on one stream with different data, then one on a second stream:
    every launch finds the ticket counters zero and leaves them zero."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d = ops.ModelDims()
    cases = [_gradients(d, 3, seed=s) for s in (11, 12, 13, 14)]
    Gs = [torch.tensor(g, device=cuda) for g, _, _ in cases]
    clips = [ops.BoundGradClip(d, 3, G, 1.0) for G in Gs]
    torch.cuda.synchronize()
    for c in clips[:3]:
        c()
    other = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(other):
        clips[3]()
    torch.cuda.synchronize()
    for c, (_, _, ref) in zip(clips, cases):
        _check_tables(c.norms.cpu().numpy(), c.scales.cpu().numpy(), ref, 1.0)


def _model(precision, cuda):
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_64env",
                      [f"model.precision={precision}"])
    return instantiate(cfg.model, device=cuda, seed=0)


def _net_buffers(m, net):
    """(params, actor image, critic image, nets) clones of the model's state for `net`."""
    na = m.n_actor
    if net == "actor":
        return m.actor_ft_params.clone(), m.packed_ft.clone(), None, 1
    if net == "critic":
        return m.critic_params.clone(), None, m.packed_critic.clone(), 2
    return m.train_params.clone(), m.packed_ft.clone(), m.packed_critic.clone(), 3


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("net", ["actor", "critic", "both"])
def test_clipped_step_equals_scale_then_step(cuda, precision, net):
    """Three consecutive steps through BoundOptimizerStep(clip_scales=the table of dppo_grad_clip_scales)
    against the same steps on G * expand(scales) (a plain torch fp32 multiply) without clip_scales, in
    the staged, fused_pack and fused_pack + clear_grads forms: parameters, moments and image bytes are
    torch.equal; with clear_grads the gradients and the clear ranges are zero afterwards and nothing
    else is touched; variables whose scale is 1.0 equal the unclipped step's result exactly."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    m = _model(precision, cuda)
    d = m.dims
    P0, ia0, ic0, nets = _net_buffers(m, net)
    n = P0.numel()
    na = m.n_actor
    sizes = _var_sizes(d, nets)
    gen = torch.Generator(device=cuda).manual_seed(7)
    G0 = torch.randn(n, device=cuda, generator=gen) * 0.05     # weights and wide biases above 1, the rest below
    M0 = torch.rand(n, device=cuda, generator=gen) * 1e-4
    V0 = torch.rand(n, device=cuda, generator=gen) * 1e-7
    _, scales = ops.grad_clip_scales(d, nets, G0, 1.0)
    torch.cuda.synchronize()
    sc = scales.cpu().numpy()
    assert 0 < int((sc == 1.0).sum()) < len(sizes), sc
    counts = torch.tensor(sizes, device=cuda)
    G_scaled = G0 * torch.repeat_interleave(scales, counts)     # expand(scales), read back from the same table
    scratch = torch.full((3, 300), 7.0, dtype=torch.float64, device=cuda)
    # the staged step of both networks packs 23 image segments, and one pack launch holds 24 jobs: its
    # gradient clear fits, three more clear ranges do not (they are the one-network steps')
    n_clear = 0 if net == "both" else 3

    def run(G_in, clip_scales, fused, clear_g):
        P, M, V, G = P0.clone(), M0.clone(), V0.clone(), G_in.clone()
        ia, ic = (None if ia0 is None else ia0.clone()), (None if ic0 is None else ic0.clone())
        ap = None if ia is None else P[:na]
        cp = None if ic is None else (P[na:] if ia is not None else P)
        step = ops.BoundOptimizerStep(d, m.precision, P, G, M, V, 0.004, 0.9, 0.999, 1e-7, "keras", ap, ia, cp, ic,
                                      defer_sampler_tables=ia is not None, fused_pack=fused, clear_grads=clear_g,
                                      clip_scales=clip_scales)
        clear = None
        scratch.fill_(7.0)
        if clear_g and n_clear:
            clear = type("C", (), {})()
            base = scratch.data_ptr()
            clear.args = ((ctypes.c_void_p * 4)(base, base + 2400, base + 4800 + 16), (ctypes.c_size_t * 4)(8, 2400, 1000), 3)
        for it in range(3):
            if clear_g and it:
                G.copy_(G_in)
            step(it + 2, 1e-3 * (it + 1), clear=clear)
        if ia is not None:
            ops.refresh_sampler_tables(ia)
        torch.cuda.synchronize()
        return P, M, V, ia, ic, G

    bounds = np.concatenate([[0], np.cumsum(sizes)])
    for variant, (fused, clear_g) in (("staged", (False, False)), ("fused", (True, False)), ("fused_clear", (True, True))):
        got = run(G0, scales, fused, clear_g)
        want = run(G_scaled, None, fused, clear_g)
        for name, a, b in zip(("params", "m", "v", "actor image", "critic image"), got[:5], want[:5]):
            assert (a is None and b is None) or torch.equal(a, b), (variant, name)
        if clear_g:
            assert int(torch.count_nonzero(got[5])) == 0
            expect = torch.full((3, 300), 7.0, dtype=torch.float64, device=cuda).view(torch.uint8).view(-1)
            for lo, nb in ((0, 8), (2400, 2400), (4816, 1000))[:n_clear]:
                expect[lo:lo + nb] = 0
            assert torch.equal(scratch.view(torch.uint8).view(-1), expect)   # the ranges zero, nothing else touched
        else:
            assert torch.equal(got[5], G0)                      # the gradients themselves are never rewritten
        plain = run(G0, None, fused, clear_g)                   # the unclipped step
        assert not torch.equal(plain[0], got[0])
        for v in np.nonzero(sc == 1.0)[0]:
            lo, hi = int(bounds[v]), int(bounds[v + 1])
            for a, b in zip(got[:3], plain[:3]):
                assert torch.equal(a[lo:hi], b[lo:hi]), (variant, int(v))


def test_clip_refusals_leave_the_parameters_alone(cuda):
    """clip_scales with l2_from_pl2, and a range that is not a whole network, raise with the library's
    message before anything is launched."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    m = _model("bf16", cuda)
    d, na = m.dims, m.n_actor
    P, img = m.actor_ft_params.clone(), m.packed_ft.clone()
    G = torch.randn(na, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3)) * 0.05
    M, V = torch.zeros(na, device=cuda), torch.zeros(na, device=cuda)
    scales = torch.full((12,), 0.5, device=cuda)
    P_before, img_before = P.clone(), img.clone()
    step = ops.BoundOptimizerStep(d, m.precision, P, G, M, V, 0.004, 0.9, 0.999, 1e-7, "keras", P, img,
                                  l2_from_pl2=True, clip_scales=scales)
    with pytest.raises(_lib.DppoError, match="DPPO_STEP_L2_FROM_PL2"):
        step(1, 1e-3)
    k = na - 4
    step = ops.BoundOptimizerStep(d, m.precision, P[:k], G[:k], M[:k], V[:k], 0.004, 0.9, 0.999, 1e-7, "keras",
                                  clip_scales=scales)
    with pytest.raises(_lib.DppoError, match="exactly"):
        step(1, 1e-3)
    with pytest.raises(_lib.DppoError, match="exactly"):      # the critic's table on the actor's range
        ops.optimizer_step(d, m.precision, P, G, M, V, 1, 1e-3, 0.004, 0.9, 0.999, 1e-7, "keras",
                           clip_scales=torch.ones(8, device=cuda))
    torch.cuda.synchronize()
    assert torch.equal(P, P_before) and torch.equal(img, img_before)
    assert int(torch.count_nonzero(M)) == 0 and int(torch.count_nonzero(V)) == 0


# The clip threshold of the agent tests, picked from the per-variable gradient norms of their workload
# (hopper cfg, fp32, n_steps 20, batch_size 200, max_grad_norm set and the reference's threshold 1.0), as
# the split path's norm kernel reported them on an MI355X over the 20 minibatches of the train iteration
# (min .. max per variable, layout order):
#   actor   time_w1 .0037-.0157  time_b1 .0013-.0058  time_w2 .0038-.0135  time_b2 .0020-.0075
#           in_w .0349-.0817  in_b .0091-.0245  l1_w .0218-.0472  l1_b .0058-.0136
#           l2_w .0215-.0503  l2_b .0083-.0229  out_w .0334-.0799  out_b .0061-.0159
#   critic  in_w .316-.763  in_b .754-1.09  l1_w .165-.376  l1_b .439-.635
#           l2_w .163-.345  l2_b .693-1.03  out_w .286-.685  out_b .480-.712
# (the data-parallel form, 40 minibatches: actor .0019-.122, the time MLP and the biases <= .031;
# critic .088-1.11). At 1.0 nothing but two critic biases is ever clipped; at 0.05 every critic variable
# is, the actor's time MLP and biases never are, and its four weight matrices come and go.
AGENT_CLIP_NORM = 0.05


def _timer_names(lib):
    names = []
    while True:
        nm = lib.dppo_kernel_timing_name(len(names))
        if not nm:
            return names
        names.append(nm.decode())


def _run_clipped_agent(tmp_path, monkeypatch, flag, cfg_name, extra, dp):
    import torch
    from diffusionpolicyoptimization_amd import _lib
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    monkeypatch.setenv("DPPO_SPLIT_UPDATE", flag)
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), cfg_name,
                      ["model.precision=fp32", "train.n_steps=20", "train.batch_size=200", "train.n_train_itr=2",
                       "train.val_freq=100", f"logdir={tmp_path}/{flag}", "train.max_grad_norm=1.0",
                       f"train.grad_clip_norm={AGENT_CLIP_NORM}"] + extra)
    a = get_class(cfg._target_)(cfg)
    assert a.max_grad_norm == 1.0 and float(a.grad_clip_norm) == AGENT_CLIP_NORM
    calls = []
    if dp:
        a.world_size = 2                          # rank 0 of 2; every reduction goes through _allreduce

        def replica_sum(t, calls=calls):
            calls.append(t.numel())
            return t.mul_(2.0)
        a._allreduce = replica_sum
    lib = _lib.load()
    names = _timer_names(lib)
    _lib.call("dppo_kernel_timing", 1)
    try:
        res = a.run()
        torch.cuda.synchronize()
        tot, cnt = np.zeros(len(names)), np.zeros(len(names), np.int64)
        _lib.call("dppo_kernel_timing_read", len(names), ctypes.c_void_p(tot.ctypes.data), ctypes.c_void_p(cnt.ctypes.data))
    finally:
        _lib.call("dppo_kernel_timing", 0)
    launches = dict(zip(names, cnt.tolist()))
    return a, res, launches, calls


def _compare_split_to_unsplit(out, keys):
    a1, r1, l1, _ = out["1"]
    a0, r0, l0, _ = out["0"]
    # the split run really took the split path, with one norm launch per half and applied minibatch
    assert "actor" in a1._bound and "clip_actor" in a1._bound and "all" not in a1._bound
    n1, n0 = a1.timing["n_updates"], a0.timing["n_updates"]
    assert n1 == n0 > 0
    assert l1["grad_clip_kernel"] == 2 * n1 and l0["grad_clip_kernel"] == 0, (l1, l0)
    assert "actor" not in a0._bound
    p1, p0 = a1.model.train_params.cpu().numpy(), a0.model.train_params.cpu().numpy()
    d = np.abs(p1 - p0)
    print("median |dparam|", float(np.median(d)), "max", float(d.max()))
    t1, t0 = ([it for it in r if not it["eval"]] for r in (r1, r0))     # the train iterations report the clip
    assert len(t1) == len(t0) > 0
    for r in (t1, t0):
        for it in r:
            print("itr", it["itr"], "grad_norm_max", it["grad_norm_max"], "grad_clipped", it["grad_clipped"])
            assert 0 < it["grad_clipped"] < 20, it["grad_clipped"]    # the clip is neither idle nor total
    assert np.median(d) < 1e-6 and d.max() < 5e-3, (float(np.median(d)), float(d.max()))
    for k in keys:
        assert abs(r1[-1][k] - r0[-1][k]) <= 1e-3 * (abs(r0[-1][k]) + 1e-3), (k, r1[-1][k], r0[-1][k])
    for i1, i0 in zip(t1, t0):      # the two paths' own reports of the last minibatch's norms agree
        assert abs(i1["grad_clipped"] - i0["grad_clipped"]) <= 1    # (a norm at the threshold may fall either way)
        assert abs(i1["grad_norm_max"] - i0["grad_norm_max"]) <= 1e-3 * i0["grad_norm_max"]


def test_clipped_split_update_matches_unsplit(cuda, tmp_path, monkeypatch):
    """train.max_grad_norm keeps the split update (critic half on the side stream, one-launch fused
    steps, pre-cleared minibatches) and trains like the unsplit path with the per-variable torch clip,
    within test_split_update_matches_fused's bounds."""
    out = {flag: _run_clipped_agent(tmp_path, monkeypatch, flag, "ft_ppo_diffusion_mlp", [], dp=False)
           for flag in ("1", "0")}
    _compare_split_to_unsplit(out, ("pg_loss", "v_loss"))


def test_clipped_split_dp_update_matches_unsplit_dp(cuda, tmp_path, monkeypatch):
    """The same under data parallelism in test_split_dp_update_matches_fused_dp's form (rank 0 of 2, an
    all-reduce that sums two identical replicas): each half's norms are taken AFTER its bucket
    all-reduce, as the reference clips the whole batch's gradient; a clip before the all-reduce would
    see half the norm and fail the comparison."""
    out = {flag: _run_clipped_agent(tmp_path, monkeypatch, flag, "ft_ppo_diffusion_mlp", [], dp=True)
           for flag in ("1", "0")}
    _compare_split_to_unsplit(out, ("pg_loss", "v_loss"))
    a1, c1, c0 = out["1"][0], out["1"][3], out["0"][3]
    assert a1.model.n_actor in c1 and a1.model.grads_ext.numel() in c0    # two buckets against one
