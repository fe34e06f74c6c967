"""Cases, inputs, float64 oracle and bounds of tests/test_lstm.py and tests/test_lstm_gpu.py.  The oracle is a loop
over t on the bf16-rounded inputs, plain or with the kernels' storage roundings (h_t, the saved gates and dgates to
bf16, all else exact).  A result must lie within 2 floor of the reference, floor = max |plain - rounded| / max
|plain|: one storage point rounding the other way moves it by at most one more ulp than the emulation did.  Only
where no rounding reaches an output (floor exactly 0: the final c under an all-zero cont) the bound is eps32.
Every case starts from a non-zero state, so cont_0 = 0 matters; T = 1 is the two-forwards case, where the carried
state is the only recurrence.  Measured on the CPU (test_recurrence_matters): on h, W_hc = 0 moves the oracle by 83
to 264 bounds where cont is not all zeros, cont forced to ones (zeros in the two-forwards case) by 80 to 497."""
import functools
import typing
import zlib

import torch

BF16, F64 = torch.bfloat16, torch.float64


class Case(typing.NamedTuple):
    name: str
    T: int
    N: int
    D: int
    H: int
    cont: str            # zero at t = 0 only ("start"), for one stream mid-sequence only ("mid"), everywhere ("zeros")
    static: int = 0      # values per stream of x_static; 0: none
    twice: bool = False  # a first forward ("start"), then the checked one with cont all ones


CASES = (Case("h8_n1", 3, 1, 8, 8, "start"),        # less than one unit tile and one K-step
         Case("h24_n16", 3, 16, 24, 24, "mid"),     # unit tail and K tail
         Case("h40_n17", 5, 17, 8, 40, "start"),    # a full K-step and a tail; a second row tile of one row
         Case("h136_n17", 3, 17, 24, 136, "mid"),   # several K-steps per wave and a tail
         Case("h136_n1_t5", 5, 1, 8, 136, "start"),
         Case("cont_zeros", 3, 16, 8, 24, "zeros"),
         Case("static", 3, 17, 8, 40, "start", static=24),
         Case("carry_t1", 1, 16, 24, 24, "start", twice=True))


@functools.lru_cache(maxsize=None)
def inputs(case) -> dict:
    """fp32 tensors, bf16-rounded but for c0 and cont: x [T, N, D], w_xc, b_c, w_hc, h0, c0, dh [T, N, H], cont."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    T, N, D, H = case.T, case.N, case.D, case.H
    r = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g)).to(BF16).float()
    i = {"x": r(T, N, D), "w_xc": r(4 * H, D, s=D ** -0.5), "b_c": r(4 * H, s=0.5), "w_hc": r(4 * H, H, s=2 * H ** -0.5),
         "h0": (2 * torch.rand(N, H, generator=g) - 1).to(BF16).float(), "c0": torch.randn(N, H, generator=g),
         "dh": r(T, N, H)}
    if case.static:
        i["xs"], i["w_xs"] = r(N, case.static), r(4 * H, case.static, s=case.static ** -0.5)
    cont = torch.ones(T, N) * (case.cont != "zeros")
    cont[0] *= case.cont != "start"
    cont[T // 2, N // 2] *= case.cont != "mid"
    if case.twice:
        i["cont_first"], cont = cont, torch.ones(T, N)
    i["cont"] = cont
    return i


def oracle(i, rounded=False, w_hc=None, cont=None, tail=None) -> dict:
    """The outputs of the last forward; ``tail(h, round)`` -> (dh, more outputs) stands for the layers above."""
    rb = (lambda t: t.to(BF16).to(F64)) if rounded else (lambda t: t)
    d = {k: v.to(F64) for k, v in i.items()}
    x, wx, wh = d["x"], d["w_xc"], d["w_hc"] if w_hc is None else w_hc.to(F64)
    (T, N, _), H = x.shape, wh.shape[1]
    stat = d["xs"] @ d["w_xs"].t() if "xs" in d else 0.0
    h, c = d["h0"], d["c0"]
    for ct in ([d["cont_first"]] if "cont_first" in d else []) + [d["cont"] if cont is None else cont.to(F64)]:
        hs, cs, gates, hcs = [], [c], [], []
        for t in range(T):
            hc = ct[t, :, None] * h
            pre = x[t] @ wx.t() + d["b_c"] + stat + hc @ wh.t()
            gi, gf, go = (torch.sigmoid(pre[:, k * H:(k + 1) * H]) for k in range(3))
            gg = torch.tanh(pre[:, 3 * H:])
            c = ct[t, :, None] * gf * c + gi * gg
            h = rb(go * torch.tanh(c))
            hs.append(h), cs.append(c), gates.append([rb(v) for v in (gi, gf, go, gg)]), hcs.append(hc)
    top, more = tail(torch.stack(hs), rb) if tail else (d["dh"], {})
    dg, dc = [None] * T, torch.zeros(N, H, dtype=F64)
    for t in range(T - 1, -1, -1):
        dh = top[t] + (ct[t + 1, :, None] * (dg[t + 1] @ wh) if t < T - 1 else 0.0)
        gi, gf, go, gg = gates[t]
        tc = torch.tanh(cs[t + 1])
        dc = dc + dh * go * (1 - tc * tc)
        dg[t] = rb(torch.cat([dc * gg * gi * (1 - gi), dc * ct[t, :, None] * cs[t] * gf * (1 - gf), dh * tc * go * (1 - go),
                              dc * gi * (1 - gg * gg)], 1))
        dc = dc * ct[t, :, None] * gf
    dg2 = torch.cat(dg)
    out = {"h": torch.stack(hs), "c": c, "dx": (dg2 @ wx).reshape(x.shape), "dw_xc": dg2.t() @ x.reshape(T * N, -1),
           "db": dg2.sum(0), "dw_hc": dg2.t() @ torch.cat(hcs), **more}
    if "xs" in d:
        out["dxs"], out["dw_xs"] = sum(dg) @ d["w_xs"], sum(dg).t() @ d["xs"]
    return out


def distance(got, want) -> float:
    """max |got - want| / max |want| (the absolute distance from an all-zero ``want``)."""
    want = want.detach().cpu().to(F64)
    return float((got.detach().cpu().to(F64).reshape(want.shape) - want).abs().max()) / (float(want.abs().max()) or 1.0)


def eps32(T, D, H) -> float:
    """fp32 arithmetic: 2^-24 per operation over sums of D + 4H terms and T steps (2e-6 to 2e-4 here)."""
    return 2.0 ** -24 * (D + 4 * H) * T


def bounds(plain, rnd, eps) -> dict:
    """2 floor per output; ``eps`` where the floor is exactly 0 and the output is not (an all-zero output: 0)."""
    floor = {k: distance(rnd[k], plain[k]) for k in plain}
    return {k: 2 * f or (eps if float(plain[k].abs().max()) else 0.0) for k, f in floor.items()}


@functools.lru_cache(maxsize=None)
def expected(case):  # (plain oracle, {output: bound})
    plain = oracle(inputs(case))
    return plain, bounds(plain, oracle(inputs(case), rounded=True), eps32(case.T, case.D, case.H))


def worst_ratio(got: dict, want: dict, bound: dict, what) -> float:
    """The largest distance / bound over the outputs, each printed (0 / 0 counts as 0)."""
    ratios = {k: distance(got[k], want[k]) / max(b, 1e-300) for k, b in bound.items()}
    print("lstm", what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    return max(ratios.values())
