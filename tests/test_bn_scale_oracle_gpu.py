"""The fused BatchNorm / Scale / ReLU kernels (csrc/kernels/bn_scale.hip) on the GPU against the fp64
oracle and the format-derived bounds of tests/bn_scale_cases.py: the five wrappers of
ops.layers_hip driven directly on [R][C] tensors, every output compared element by element (per
channel, never normalised by a global maximum), the gradient flags, the refusals, the workspace
size and bitwise repeatability.  Each comparison prints ``RATIO quantity type case value`` (error
over bound, <= 1 passes) before it asserts."""
import pytest
import torch

import bn_scale_cases as bc

pytestmark = pytest.mark.gpu


def _dev(t, gpu, misaligned=False):
    """t on the device; misaligned: as a contiguous view one element into a larger buffer."""
    if t is None:
        return None
    if not misaligned:
        return t.to(gpu)
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=gpu)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and buf.data_ptr() % 16 == 0
    return v


def _stats(lh, ref, gpu):
    k, i = ref.k, ref.i
    if k.mode == bc.BN_BATCH:
        return (lh.BN_BATCH, ref.sa.to(gpu), ref.sb.to(gpu), None, i.eps)
    if k.mode == bc.BN_GLOBAL:
        return (lh.BN_GLOBAL, ref.sa.to(gpu), ref.sb.to(gpu), ref.sf.to(gpu), i.eps)
    return lh.NO_STATS


def run(gpu, case, dtype, cfg):
    """Every output of one configuration, from the wrappers: the statistics (batch configurations),
    the forward, pass 1 with both gradients stored, accumulated and each skipped in turn, pass 2."""
    from sparknet_amd.ops import layers_hip as lh
    ref = bc.reference(case, dtype, cfg)
    i, k, R, C = ref.i, ref.k, case.R, case.C
    x, dy = _dev(ref.x, gpu, case.view == "x"), _dev(i.dy, gpu, case.view == "dy")
    gamma, beta = _dev(ref.gamma, gpu), _dev(ref.beta, gpu)
    o = {}
    if k.mode == bc.BN_BATCH:
        o["rm"], o["rv"], o["rf"] = i.rm0.to(gpu), i.rv0.to(gpu), i.rf0.to(gpu)
        o["mean"], o["var"], o["inv"] = lh.bn_stats(x, R, C, i.eps, (o["rm"], o["rv"], o["rf"]), i.frac, i.unbias)
        o["bare"] = lh.bn_stats(x, R, C, i.eps)  # without running blobs
    stats = _stats(lh, ref, gpu)
    y = o["y"] = lh.bn_fwd(x, R, C, stats, gamma, beta, k.relu)
    full = lambda: torch.full((C,), bc.PREFILL, device=gpu)
    for flag, sfx in ((lh.GRAD_STORE, ""), (lh.GRAD_ACC, "_acc")):
        o["dgamma" + sfx], o["dbeta" + sfx] = full(), full()
        coef = lh.bn_bwd_reduce(dy, x, y, R, C, stats, k.relu, o["dgamma" + sfx], flag, o["dbeta" + sfx], flag)
        o["coef" + sfx] = coef
    o["g_only"], o["b_skipped"], o["b_only"], o["g_skipped"] = full(), full(), full(), full()
    o["coef_g"] = lh.bn_bwd_reduce(dy, x, y, R, C, stats, k.relu, o["g_only"], lh.GRAD_STORE, o["b_skipped"], lh.GRAD_SKIP)
    # without batch statistics this is the need_x = 0 call: x is not read
    o["coef_b"] = lh.bn_bwd_reduce(dy, x, y, R, C, stats, k.relu, o["g_skipped"], lh.GRAD_SKIP, o["b_only"], lh.GRAD_STORE)
    assert lh.bn_bwd_reduce(dy, x, y, R, C, stats, k.relu, dbeta=full(), bflag=lh.GRAD_STORE, want_coef=False) is None
    o["dx"] = lh.bn_bwd_dx(dy, x, y, R, C, stats, k.relu, gamma, o["coef"])
    torch.cuda.synchronize()
    return ref, o


def _check(ref, o, case, dtype, cfg, names):
    bad = {}
    for q in names:
        w = bc.worst(o[q], getattr(ref, q), ref.bound[q])
        print("RATIO", q, bc.dname(dtype), f"{case.name}-{cfg}", f"{w:.4g}")
        if not w <= 1.0:
            bad[q] = w
    assert not bad, bad


@pytest.mark.parametrize("case, dtype, cfg", bc.PARAMS, ids=bc.PARAM_IDS)
def test_wrappers_meet_the_oracle(gpu, case, dtype, cfg):
    from sparknet_amd.ops import layers_hip as lh
    assert (lh.BN_NONE, lh.BN_BATCH, lh.BN_GLOBAL) == (bc.BN_NONE, bc.BN_BATCH, bc.BN_GLOBAL)
    ref, o = run(gpu, case, dtype, cfg)
    C = case.C
    batch = ref.k.mode == bc.BN_BATCH
    names = ["y", "dgamma", "dbeta", "dgamma_acc", "dbeta_acc", "dx"]
    assert o["y"].dtype == dtype and o["dx"].dtype == dtype and o["y"].shape == o["dx"].shape == (case.R, C)
    if batch:
        names = ["mean", "var", "inv", "rm", "rv", "rf"] + names + ["c1", "c2"]
        o["c1"], o["c2"] = o["coef"][:C], o["coef"][C:]
        assert all(torch.equal(a, b) for a, b in zip(o["bare"], (o["mean"], o["var"], o["inv"])))
    else:  # pass 2 takes no coefficients from pass 1
        assert not bool(o["coef"].any())
    assert o["coef"].shape == (2 * C,)
    _check(ref, o, case, dtype, cfg, names)
    # one gradient skipped while the other stores: the stored one is within its bound and, like the
    # coefficients, the same bits (but for a misaligned x that the call without dgamma does not read:
    # that call runs on vector lanes, in another order); the skipped buffer is untouched
    prefill = torch.full((C,), bc.PREFILL, device=gpu)
    for q, name in (("g_only", "dgamma"), ("b_only", "dbeta")):
        assert bc.worst(o[q], getattr(ref, name), ref.bound[name]) <= 1.0, q
    assert torch.equal(o["g_only"], o["dgamma"])
    assert torch.equal(o["b_only"], o["dbeta"]) or (case.view == "x" and not batch)
    assert torch.equal(o["b_skipped"], prefill) and torch.equal(o["g_skipped"], prefill)
    assert torch.equal(o["coef_acc"], o["coef"]) and torch.equal(o["coef_g"], o["coef"])
    assert torch.equal(o["coef_b"], o["coef"])


@pytest.mark.parametrize("case, dtype, cfg", [p for p in bc.PARAMS if bc.CONFIGS[p[2]].mode == bc.BN_BATCH],
                         ids=[i for i, p in zip(bc.PARAM_IDS, bc.PARAMS) if bc.CONFIGS[p[2]].mode == bc.BN_BATCH])
def test_forward_on_the_kernels_own_statistics(gpu, case, dtype, cfg):
    """The chain as the layer runs it: bn_fwd on the mean and inv_std that bn_stats wrote, within the
    forward bound plus what the bounds of mean and inv_std propagate (the large-mean case too)."""
    from sparknet_amd.ops import layers_hip as lh
    ref = bc.reference(case, dtype, cfg)
    x = _dev(ref.x, gpu, case.view == "x")
    mean, _, inv = lh.bn_stats(x, case.R, case.C, ref.i.eps)
    y = lh.bn_fwd(x, case.R, case.C, (lh.BN_BATCH, mean, inv, None, ref.i.eps), _dev(ref.gamma, gpu), _dev(ref.beta, gpu),
                  False)
    w = bc.worst(y, ref.z, ref.bz + (0.0 if dtype == bc.F32 else bc.U16) * ref.z.abs() + ref.own)
    print("RATIO", "y_own", bc.dname(dtype), f"{case.name}-{cfg}", f"{w:.4g}")
    assert w <= 1.0


@pytest.mark.parametrize("case", bc.DET_CASES, ids=[c.name for c in bc.DET_CASES])
def test_two_runs_are_bitwise_equal(gpu, case):
    for cfg in bc.configs(case):
        (_, a), (_, b) = run(gpu, case, bc.BF16, cfg), run(gpu, case, bc.BF16, cfg)
        for q in a:
            pair = zip(a[q], b[q]) if isinstance(a[q], tuple) else ((a[q], b[q]),)
            assert all(torch.equal(s, t) for s, t in pair), (cfg, q)


@pytest.mark.parametrize("case", bc.CASES, ids=[c.name for c in bc.CASES])
def test_workspace_size(gpu, case):
    from sparknet_amd.ops import layers_hip as lh
    for dtype in case.dtypes:
        part, n = lh._bn_part(torch.empty(0, dtype=dtype, device=gpu), case.R, case.C)
        assert n == part.numel() == bc.part_floats(case, dtype)


def test_refusals_raise_and_launch_nothing(gpu):
    from sparknet_amd.ops import layers_hip as lh
    case = bc.BY_NAME["16x10"]
    ref = bc.reference(case, bc.BF16, "batch-relu")
    R, C = case.R, case.C
    x, dy = ref.x.to(gpu), ref.i.dy.to(gpu)
    mean, inv = ref.sa.to(gpu), ref.sb.to(gpu)
    y = lh.bn_fwd(x, R, C, (lh.BN_BATCH, mean, inv, None, ref.i.eps), None, None, True)
    seven = lambda n, dt=torch.float32: torch.full((n,), bc.PREFILL, dtype=dt, device=gpu)
    part, dg, db, coef, out = seven(4 * C), seven(C), seven(C), seven(2 * C), seven(R * C, torch.bfloat16)
    with pytest.raises(RuntimeError, match="code 2"):  # need_x = 0 with a gradient of gamma
        lh.call("bn_bwd_reduce", dy, None, y, 0, R, C, None, None, None, 0.0, lh.BN_NONE, 1, 0, part, part.numel(), dg,
                lh.GRAD_STORE, db, lh.GRAD_STORE, coef)
    with pytest.raises(RuntimeError, match="code 2"):  # need_x = 0 with batch statistics
        lh.call("bn_bwd_reduce", dy, None, y, 0, R, C, mean, inv, None, ref.i.eps, lh.BN_BATCH, 1, 0, part, part.numel(),
                None, lh.GRAD_SKIP, db, lh.GRAD_STORE, coef)
    with pytest.raises(RuntimeError, match="code 2"):  # batch statistics without the coefficients of pass 1
        lh.call("bn_bwd_dx", dy, x, y, out, 0, R, C, mean, inv, None, ref.i.eps, lh.BN_BATCH, 1, None, None)
    with pytest.raises(RuntimeError, match="code 2"):
        lh.bn_bwd_dx(dy, x, y, R, C, (lh.BN_BATCH, mean, inv, None, ref.i.eps), True, None, None)
    with pytest.raises(RuntimeError, match="code 3"):  # a workspace smaller than the plan needs
        lh.call("bn_bwd_reduce", dy, x, y, 0, R, C, mean, inv, None, ref.i.eps, lh.BN_BATCH, 1, 1, part, 2 * C - 1, dg,
                lh.GRAD_STORE, db, lh.GRAD_STORE, coef)
    for r, c in ((0, C), (R, 0), (-1, C), (1, 2147483647 // 8 + 1)):  # bad geometry
        with pytest.raises(ValueError):
            lh._bn_part(x, r, c)
        with pytest.raises(ValueError):
            lh.bn_stats(x, r, c, 1e-5)
        with pytest.raises(RuntimeError, match="code 3"):
            lh.call("bn_fwd", x, out, 0, r, c, mean, inv, None, ref.i.eps, lh.BN_BATCH, None, None, 0)
        with pytest.raises(RuntimeError, match="code 3"):
            lh.call("bn_bwd_dx", dy, x, y, out, 0, r, c, mean, inv, None, ref.i.eps, lh.BN_BATCH, 1, None, coef)
        with pytest.raises(RuntimeError, match="code 3"):
            lh.call("bn_stats", x, 0, r, c, part, part.numel(), 1e-5, dg, None, db, None, None, None, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="code 3"):
        lh.call("axis_scale_bias", x, out, 0, 1, 1, None, None, 0)
    torch.cuda.synchronize()
    for t in (part, dg, db, coef, out):  # nothing was written
        assert bool((t == bc.PREFILL).all())


@pytest.mark.parametrize("dtype", bc.BOTH, ids=("bf16", "fp32"))
@pytest.mark.parametrize("A", (1, 5))
@pytest.mark.parametrize("inner", (1, 3, 49))
def test_axis_scale_bias(gpu, inner, A, dtype):
    from sparknet_amd.ops import layers_hip as lh
    x, s, b = bc.axis_inputs(3, A, inner, dtype)
    xd = x.to(gpu)
    for use_s, use_b in ((True, True), (True, False), (False, True)):
        ss, bb = (s if use_s else None), (b if use_b else None)
        y = lh.axis_scale_bias(xd, _dev(ss, gpu), _dev(bb, gpu), A, inner)
        assert y.dtype == dtype and y.shape == x.shape
        w = bc.worst(y.reshape(-1), *bc.axis_bound(x, ss, bb, A, inner, dtype))
        print("RATIO", "axis", bc.dname(dtype), f"{A}x{inner}-{use_s}-{use_b}", f"{w:.4g}")
        assert w <= 1.0, (use_s, use_b)
