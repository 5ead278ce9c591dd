"""QRNN fo-pool scan, fused AdamW, seeded DropConnect, embedding
gather/scatter and AR/TAR kernels vs the fp64 references of
tests/train_ref.py.

Every kernel runs through lib.* and through its Python wrapper. QRNN and
AdamW are held to K * E + one rounding of the storage format (K = 2,
E = max|model - exact| from the CPU; fp32 QRNN tensors to 2e-4 relative to
max(1, max|exact|)); the embedding scatter and the AR/TAR sums to the fp32
summation bound; the AR/TAR gradients to 4 fp32 ulps plus half an ulp of the
storage type; DropConnect and the embedding gather to the reference's bits.
tests/test_train_ref.py shows each bound is at least 2x below what the wrong
variants of train_ref cause. The bindings must refuse mistyped or misshapen
arguments before anything is launched; only refusals whose launch would
stay inside every buffer are tried.

Measured on MI355X, worst err/allowed over each group's cases:
  QRNN scan (lib.*)          h      c      act    dgates dc0
  bf16                       0.33   0.33   0.33   0.45   0.41
  bf16, pre-activations x8   0.33   0.33   0.33   0.50   0.38
  fp32 (plain and x8)        0.001  0.001  0.000  0.002  0.001
  fo_pool autograd, bf16     0.33   0.18   -      0.42   0.43   (c is cT)
  4 + 5 windows, bf16        0.33   0.28   -      -      -
  fp32 windows: h bit-identical to the single window.
  The fp32 figures are small because that bound is the suite's 2e-4, not
  the modelled roundings; the bf16 ones sit where the model does.

  AdamW                      master exp_avg exp_avg_sq
  fp32 parameter             0.49   0.51    0.49
  bf16 parameter + master    0.49   0.46    0.54
  64 sub-ulp steps           0.49   -       -
  A bf16 p equalled master.to(bfloat16) in every case.

  embedding scatter          dW fp32 out   wgrad through autograd
  fp32 / bf16 gout           0.99 / 0.95   0.02 / 0.95
  Near 1 because a row looked up twice has a bound of one fp32 rounding
  of the sum; rows looked up once were exact, as the bound demands.

  AR/TAR                     sum sq  sum diff  reg    dout   dr
  fp32                       0.001   0.002     0.001  0.24   0.20
  fp32, second trip          0.018   0.009     0.010  0.20   0.37
  bf16                       0.002   0.002     0.001  0.99   1.00
  bf16, second trip          0.002   0.008     -      1.00   1.00
  The bf16 gradients sit at 1 because their bound is one bf16 rounding.

DropConnect (apply, grad_ and the autograd function) and the embedding
gather matched the host references bit for bit, kept values included: no
kernel differed by an ulp, and no kernel needed a fix.
"""
import math

import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32


def _lib():
    from code_intelligence_amd.ops import extension as ext
    return ext.require()


def _check(name, tag, got, exact, allowed):
    r = R.ratio(got.detach().cpu(), exact, allowed)
    print(f"RATIO {name} {tag}: {r:.3f}")
    assert r <= 1.0, (name, tag, r)


def _same_bits(got, want, what):
    got, want = R.bits(got.detach().cpu()).flatten(), R.bits(want).flatten()
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, (what, bad.numel(), bad[:8].tolist(),
                              got[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- 1. QRNN fo-pool scan ---------------------------------------------------

@pytest.mark.parametrize("case", R.qrnn_scaled_cases(), ids=R.qrnn_scaled_id)
def test_qrnn_scan_vs_fp64(case):
    """lib.qrnn_fo_pool_fwd / _bwd at one and several workgroups, vector and
    scalar kernels, T = 1 and saturated gates. The forward gets a clone (it
    consumes its input) and must leave the activated gates in it; the
    backward reads what the forward stored, as in training. (None of the
    bindings in this file takes an output buffer that could be pre-filled:
    each allocates its own.)"""
    lib = _lib()
    c = R.qrnn_case(*case)
    tag = R.qrnn_scaled_id(case)
    inp, ex, al = c["inp"], c["exact"], c["allowed"]
    gates = inp["gates"].to(DEV).clone()
    c0, dh, dcT = (inp[k].to(DEV) for k in ("c0", "dh", "dcT"))
    h, cs = lib.qrnn_fo_pool_fwd(gates, c0)
    dgates, dc0 = lib.qrnn_fo_pool_bwd(gates, cs, c0, dh, dcT)
    got = dict(h=h, c=cs, act=gates, dgates=dgates, dc0=dc0)
    for k in R.QRNN_KEYS:
        assert torch.isfinite(got[k].float()).all(), k
        _check(f"qrnn.{k}", tag, got[k], ex[k], al[k])


@pytest.mark.parametrize("dt", [F32, BF16], ids=R.dt_id)
@pytest.mark.parametrize("loss_on", ["h", "h_cT"])
def test_fo_pool_autograd_vs_fp64(dt, loss_on):
    """Through fo_pool: a loss on h alone reaches backward with dcT None."""
    from code_intelligence_amd.ops.qrnn import fo_pool
    inp = dict(R.qrnn_inputs(5, 7, 12, dt))
    if loss_on == "h":
        inp["dcT"] = torch.zeros_like(inp["dcT"])
    ev = R.qrnn_eval(inp)
    pre = inp["gates"].to(DEV).requires_grad_(True)
    c0 = inp["c0"].to(DEV).requires_grad_(True)
    h, cT = fo_pool(pre.clone(), c0)
    if loss_on == "h":
        h.backward(inp["dh"].to(DEV))
    else:
        torch.autograd.backward([h, cT], [inp["dh"].to(DEV),
                                          inp["dcT"].to(DEV)])
    tag = f"{R.dt_id(dt)}-{loss_on}"
    ex, al = ev["exact"], ev["allowed"]
    _check("fo_pool.h", tag, h, ex["h"], al["h"])
    _check("fo_pool.cT", tag, cT, ex["c"][:, -1], al["c"][:, -1])
    _check("fo_pool.dgates", tag, pre.grad, ex["dgates"], al["dgates"])
    _check("fo_pool.dc0", tag, c0.grad, ex["dc0"], al["dc0"])


@pytest.mark.parametrize("dt", [F32, BF16], ids=R.dt_id)
def test_qrnn_windows_carry_state(dt):
    """T = 9 as one window and as 4 + 5 with cT carried. In fp32 c is stored
    unrounded and the operations are the same, so h must be bit-identical;
    in bf16 the carried c is rounded once more and only the bound applies."""
    lib = _lib()
    B, T, H = 3, 9, 12
    c = R.qrnn_case(B, T, H, dt)
    gates = c["inp"]["gates"].to(DEV)
    c0 = c["inp"]["c0"].to(DEV)
    h1, _ = lib.qrnn_fo_pool_fwd(gates.clone(), c0)
    ha, ca = lib.qrnn_fo_pool_fwd(gates[:, :4].contiguous(), c0)
    hb, cb = lib.qrnn_fo_pool_fwd(gates[:, 4:].contiguous(),
                                  ca[:, -1].contiguous())
    h2 = torch.cat([ha, hb], 1)
    tag = R.dt_id(dt)
    _check("qrnn_windows.h", tag, h2, c["exact"]["h"], c["allowed"]["h"])
    _check("qrnn_windows.cT", tag, cb[:, -1], c["exact"]["c"][:, -1],
           c["allowed"]["c"][:, -1])
    if dt == F32:
        _same_bits(h2, h1.cpu(), "h of 4 + 5 vs one window")


@pytest.mark.parametrize("bad", ["dh_fp32", "dcT_fp32", "c_fp32", "dh_long",
                                 "dcT_3d"])
def test_qrnn_bwd_refuses_bad_arguments(bad):
    """Each bad tensor is larger than the expected one, so a launch would
    have stayed inside every buffer; the binding raises before it."""
    lib = _lib()
    B, T, H = 2, 3, 8
    inp = R.qrnn_inputs(B, T, H, BF16)
    gates = inp["gates"].to(DEV)
    c0, dh, dcT = (inp[k].to(DEV) for k in ("c0", "dh", "dcT"))
    _, cs = lib.qrnn_fo_pool_fwd(gates, c0)
    if bad == "dh_fp32":
        dh = dh.float()
    elif bad == "dcT_fp32":
        dcT = dcT.float()
    elif bad == "c_fp32":
        cs = cs.float()
    elif bad == "dh_long":
        dh = torch.cat([dh, dh[:, :1]], 1).contiguous()
    elif bad == "dcT_3d":
        dcT = dcT[None].expand(2, B, H).contiguous()
    with pytest.raises(RuntimeError):
        lib.qrnn_fo_pool_bwd(gates, cs, c0, dh, dcT)
    torch.cuda.synchronize()


# ---- 2. fused AdamW ---------------------------------------------------------

def _bias_corrections(step):
    b1, b2 = R.ADAM_BETAS
    return 1 - b1 ** step, 1 - b2 ** step


@pytest.mark.parametrize("case", R.adam_cases(), ids=R.adam_case_id)
def test_adamw_kernel_vs_fp64(case):
    """lib.fused_adamw step by step with fresh gradients: master and both
    moments against fp64; a bf16 parameter must be its master's rounding."""
    lib = _lib()
    n, dt, steps, wd, eps = case
    c = R.adam_case(*case)
    tag = R.adam_case_id(case)
    p = c["p0"].to(DEV).clone()
    master = p if dt == F32 else p.float()
    ea, eas = torch.zeros_like(master), torch.zeros_like(master)
    for i, g in enumerate(c["grads"]):
        bc1, bc2 = _bias_corrections(i + 1)
        lib.fused_adamw([p], [g.to(DEV)], [master], [ea], [eas], R.ADAM_LR,
                        *R.ADAM_BETAS, eps, wd, bc1, bc2)
    got = dict(master=master, exp_avg=ea, exp_avg_sq=eas)
    for k in R.ADAM_KEYS:
        _check(f"adamw.{k}", tag, got[k], c["exact"][k], c["allowed"][k])
    _same_bits(p, master.to(dt).cpu(), "p vs master")


def test_adamw_accumulates_steps_below_a_bf16_ulp():
    """p = 1.0 in bf16, gradient 1, lr = 1e-4: each step moves the master by
    lr, below half a bf16 ulp (1.95e-3). After 64 steps p has left 1.0 and
    is the rounding of the fp64 result."""
    from code_intelligence_amd.ops.adam import FusedAdamW
    S = R.SUBULP
    exact, allowed = R.subulp_exact()
    p = torch.ones(S["n"], dtype=BF16, device=DEV).requires_grad_(True)
    opt = FusedAdamW([p], lr=S["lr"], betas=R.ADAM_BETAS, eps=S["eps"],
                     weight_decay=S["wd"])
    for _ in range(S["steps"]):
        p.grad = torch.ones_like(p)
        opt.step()
    master = opt.state[p]["master"]
    assert master.dtype == F32
    _check("adamw.master", "subulp", master, exact, allowed)
    assert (p.detach() != 1.0).all()
    _same_bits(p, exact.to(BF16), "p vs rounded fp64 master")


@pytest.mark.parametrize("dt", [F32, BF16], ids=R.dt_id)
def test_adamw_groups_parameters_by_their_own_step_count(dt):
    """FusedAdamW.step with a parameter whose grad is None on odd steps:
    each follows its own bias correction."""
    from code_intelligence_amd.ops.adam import FusedAdamW
    case = R.two_param_case(dt)
    ps = [p.to(DEV).clone().requires_grad_(True) for p in case["p0"]]
    opt = FusedAdamW(ps, lr=R.ADAM_LR, betas=R.ADAM_BETAS, eps=1e-8,
                     weight_decay=0.1)
    for gs in case["grad_steps"]:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(DEV)
        opt.step()
    assert [opt.state[p]["step"] for p in ps] == [6, 3]
    for k, p in enumerate(ps):
        master = opt.state[p]["master"]
        _check("adamw.master", f"{R.dt_id(dt)}-two-params-{k}", master,
               case["exact"][k], case["allowed"][k])
        _same_bits(p, master.detach().to(dt).cpu(), "p vs master")


@pytest.mark.parametrize("bad", ["grad_fp32", "grad_long", "state_long"])
def test_adamw_refuses_bad_arguments(bad):
    """An fp32 gradient for a bf16 parameter, a longer gradient and a longer
    moment: nothing may be updated, the second parameter included."""
    lib = _lib()
    n = 40
    p0, grads = R.adam_inputs(n, BF16, 1, 1e-8)
    ps = [p0.to(DEV).clone(), p0.to(DEV).clone()]
    gs = [grads[0].to(DEV), grads[0].to(DEV)]
    ms = [p.float() for p in ps]
    eas = [torch.zeros_like(m) for m in ms]
    eass = [torch.zeros_like(m) for m in ms]
    if bad == "grad_fp32":
        gs[1] = gs[1].float()
    elif bad == "grad_long":
        gs[1] = torch.cat([gs[1], gs[1]])
    elif bad == "state_long":
        eass[1] = torch.zeros(2 * n, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError):
        lib.fused_adamw(ps, gs, ms, eas, eass, 1e-3, 0.9, 0.99, 1e-8, 0.1,
                        0.1, 0.01)
    torch.cuda.synchronize()
    for p, m in zip(ps, ms):
        _same_bits(p, p0, "parameter after a refusal")
        _same_bits(m, p0.float(), "master after a refusal")


# ---- 3. DropConnect, bit for bit --------------------------------------------

def _dc_shapes():
    return [(n,) for n in R.DC_NS] + [(132, 33)]


@pytest.mark.parametrize("shape", _dc_shapes(), ids=str)
@pytest.mark.parametrize("dt", [F32, BF16], ids=R.dt_id)
def test_dropconnect_matches_host_hash(dt, shape):
    """dropconnect_apply into a fresh tensor and dropconnect_grad_ in place:
    mask, kept values and +0.0 where dropped, over vector body and tail."""
    lib = _lib()
    v = R.dc_input(math.prod(shape), dt).reshape(shape)
    for seed in R.DC_SEEDS:
        for p in R.DC_PS:
            want = R.dc_apply(v, seed, p)
            what = (shape, seed, p)
            _same_bits(lib.dropconnect_apply(v.to(DEV), seed, p), want, what)
            g = v.to(DEV).clone()
            lib.dropconnect_grad_(g, seed, p)
            _same_bits(g, want, what)


@pytest.mark.parametrize("dt", [F32, BF16], ids=R.dt_id)
def test_dropconnect_function_masks_grad_like_forward(dt):
    """_DropConnectFunction on a transposed, non-contiguous weight: elements
    are numbered in the contiguous order of w's shape, and the gradient
    comes back under the mask of the forward."""
    from code_intelligence_amd.ops.dropout import _DropConnectFunction
    seed, p = 12345, 0.5
    base = R.dc_input(33 * 132, dt).reshape(33, 132)
    w = base.to(DEV).t().requires_grad_(True)           # (132, 33)
    assert not w.is_contiguous()
    g = R.dc_input(132 * 33 + 1, dt)[1:].reshape(132, 33)
    out = _DropConnectFunction.apply(w, p, seed)
    out.backward(g.to(DEV))
    _same_bits(out, R.dc_apply(base.t().contiguous(), seed, p), "forward")
    _same_bits(w.grad, R.dc_apply(g, seed, p), "grad")


# ---- 4. embedding gather / scatter ------------------------------------------

def _mask_dev(inp):
    return inp["mask"].to(DEV)


@pytest.mark.parametrize("case", R.emb_cases(), ids=R.emb_case_id)
def test_emb_gather_bit_for_bit(case):
    from code_intelligence_amd.ops.embedding import _EmbGatherFunction
    lib = _lib()
    inp = R.emb_inputs(*case)
    want = R.gather_exact(inp["w"], inp["ids"], inp["mask"])
    w, ids = inp["w"].to(DEV), inp["ids"].to(DEV)
    got = lib.emb_gather(w, ids, _mask_dev(inp))
    assert got.shape == want.shape
    _same_bits(got, want, "lib.emb_gather")
    got = _EmbGatherFunction.apply(w, ids, _mask_dev(inp), R.EMB_PAD)
    _same_bits(got, want, "_EmbGatherFunction")


def test_embedding_row_dropout_without_mask_is_a_copy():
    from code_intelligence_amd.ops.embedding import embedding_row_dropout
    inp = R.emb_inputs((3, 4, 25), 48, BF16, False)
    got = embedding_row_dropout(inp["w"].to(DEV), inp["ids"].to(DEV), 0.0,
                                False, None)
    _same_bits(got, inp["w"][inp["ids"]], "unmasked gather")


@pytest.mark.parametrize("pad", [R.EMB_PAD, -1], ids=["pad1", "nopad"])
@pytest.mark.parametrize("case", R.emb_cases(), ids=R.emb_case_id)
def test_emb_scatter_vs_fp64(case, pad):
    """A transposed gout; pad = -1 is what ops/embedding.py passes without a
    padding index. Rows never looked up and the pad row are exactly 0."""
    lib = _lib()
    inp = R.emb_inputs(*case)
    exact, allowed = R.scatter_exact(inp["gout"], inp["ids"], inp["mask"],
                                     R.EMB_V, pad)
    gout = inp["gout"].to(DEV).transpose(0, -1).contiguous().transpose(0, -1)
    assert not gout.is_contiguous()
    dw = lib.emb_scatter(gout, inp["ids"].to(DEV), _mask_dev(inp), R.EMB_V,
                         pad)
    assert dw.dtype == F32 and dw.shape == exact.shape
    _check("emb_scatter.dw", f"{R.emb_case_id(case)}-pad{pad}", dw, exact,
           allowed)
    assert (dw[2] == 0).all()
    if pad >= 0:
        assert (dw[pad] == 0).all()


@pytest.mark.parametrize("dt", [F32, BF16], ids=R.dt_id)
def test_emb_scatter_all_tokens_on_one_row(dt):
    """300 atomic adds per element of a single row, held to the summation
    bound; through autograd the weight gradient is rounded to the table's
    dtype once more."""
    from code_intelligence_amd.ops.embedding import _EmbGatherFunction
    lib = _lib()
    shape, E, _, masked = R.EMB_SINGLE_ROW
    inp = R.emb_inputs(shape, E, dt, masked, single_row=3)
    exact, allowed = R.scatter_exact(inp["gout"], inp["ids"], inp["mask"],
                                     R.EMB_V, R.EMB_PAD)
    ids, gout = inp["ids"].to(DEV), inp["gout"].to(DEV)
    dw = lib.emb_scatter(gout, ids, _mask_dev(inp), R.EMB_V, R.EMB_PAD)
    _check("emb_scatter.dw", f"{R.dt_id(dt)}-one-row", dw, exact, allowed)
    assert (dw[:3] == 0).all() and (dw[4:] == 0).all()
    w = inp["w"].to(DEV).requires_grad_(True)
    _EmbGatherFunction.apply(w, ids, _mask_dev(inp), R.EMB_PAD).backward(gout)
    assert w.grad.dtype == dt
    _check("emb_scatter.wgrad", f"{R.dt_id(dt)}-one-row", w.grad, exact,
           allowed + R.half_ulp(exact, dt))


@pytest.mark.parametrize("bad", ["mask_fp64", "mask_long", "mask_2d_long"])
@pytest.mark.parametrize("op", ["gather", "scatter"])
def test_emb_refuses_bad_rowmask(op, bad):
    """An fp64 row mask of length V and fp32 masks of 2V values: each holds
    at least V * 4 bytes, so a launch would have stayed inside it."""
    lib = _lib()
    inp = R.emb_inputs((2, 4), 64, BF16, True)
    V = R.EMB_V
    mask = {"mask_fp64": inp["mask"].double(),
            "mask_long": inp["mask"].repeat(2),
            "mask_2d_long": inp["mask"].repeat(2).reshape(2, V)}[bad].to(DEV)
    w, ids, gout = (inp[k].to(DEV) for k in ("w", "ids", "gout"))
    with pytest.raises(RuntimeError):
        if op == "gather":
            lib.emb_gather(w, ids, mask)
        else:
            lib.emb_scatter(gout, ids, mask, V, R.EMB_PAD)
    torch.cuda.synchronize()


# ---- 5. AR/TAR --------------------------------------------------------------

def _dloss():
    return torch.full((1,), R.ARTAR_DLOSS, dtype=F32, device=DEV)


@pytest.mark.parametrize("case", R.ARTAR_CASES, ids=lambda c: c[0])
def test_artar_kernels_vs_fp64(case):
    """lib.artar_forward / artar_backward: scalar tails, n_out != n_r,
    T = 2, dloss != 1 and (fp32) the second grid-stride trip of every
    loop."""
    lib = _lib()
    name = case[0]
    c = R.artar_case(name)
    ex, al = c["exact"], c["allowed"]
    out, r = c["out"].to(DEV), c["r"].to(DEV)
    acc = lib.artar_forward(out, r)
    _check("artar.sum_sq", name, acc[0], ex["sq"], al["sq"])
    _check("artar.sum_diff", name, acc[1], ex["df"], al["df"])
    dout, dr = lib.artar_backward(out, r, _dloss(), c["ca"], c["cb"])
    _check("artar.dout", name, dout, ex["dout"], al["dout"])
    _check("artar.dr", name, dr, ex["dr"], al["dr"])


@pytest.mark.parametrize("case", R.ARTAR_CASES, ids=lambda c: c[0])
def test_artar_loss_vs_fp64(case):
    """artar_loss on r as the transpose view of time-major storage; the
    scalar is the two sums scaled in fp32 (4 more roundings)."""
    from code_intelligence_amd.ops.artar import artar_loss
    name = case[0]
    c = R.artar_case(name)
    ex, al = c["exact"], c["allowed"]
    out = c["out"].to(DEV).reshape(1, 1, -1).requires_grad_(True)
    r = c["r"].to(DEV).transpose(0, 1).requires_grad_(True)
    reg = artar_loss(out, r, R.ARTAR_ALPHA, R.ARTAR_BETA)
    assert "ARTAR" in type(reg.grad_fn).__name__
    (reg * R.ARTAR_DLOSS).backward()
    wa, wb = c["ca"] / 2, c["cb"] / 2                 # alpha / n, beta / m
    want = wa * ex["sq"] + wb * ex["df"]
    allowed = wa * al["sq"] + wb * al["df"] + 4 * R.U32 * want
    _check("artar_loss.reg", name, reg, want, allowed)
    _check("artar_loss.dout", name, out.grad.reshape(-1), ex["dout"],
           al["dout"])
    _check("artar_loss.dr", name, r.grad.transpose(0, 1), ex["dr"], al["dr"])


def test_artar_bf16_second_grid_stride_trip():
    """bf16 takes a second trip only past 8192 * 256 * 8 = 16 777 216
    elements. Both sums over everything; the gradients on windows at the
    start, around the stride and the time-row boundaries, and at the end."""
    lib = _lib()
    b = R.artar_big_case()
    out, r = b["out"].to(DEV), b["r"].to(DEV)
    acc = lib.artar_forward(out, r).cpu()
    for k, i in (("sq", 0), ("df", 1)):
        _check(f"artar.sum_{k}", "bf16-second-trip", acc[i],
               torch.tensor(b[k], dtype=torch.float64), b["rel"][k] * b[k])
    dout, dr = lib.artar_backward(out, r, _dloss(), b["ca"], b["cb"])
    for name, got, wins in (("dout", dout, b["dout"]), ("dr", dr, b["dr"])):
        flat = got.reshape(-1)
        worst = 0.0
        for (lo, hi), (exact, allowed) in wins.items():
            worst = max(worst, R.ratio(flat[lo:hi].cpu(), exact, allowed))
        print(f"RATIO artar.{name} bf16-second-trip: {worst:.3f}")
        assert worst <= 1.0, (name, worst)
