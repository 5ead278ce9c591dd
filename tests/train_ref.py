"""fp64 references for the kernels of a training step that are not the LSTM
or the CE: the QRNN fo-pool scan, fused AdamW, seeded DropConnect, the
embedding gather/scatter and the AR/TAR regulariser (plain torch and numpy,
no project code, no GPU).

Per kernel: an ``*_exact`` function (fp64 on the dtype-rounded inputs), where
the kernel stores intermediate values a ``*_model`` function (the same fp64
arithmetic with those storage roundings), and ``wrong=<name>`` variants:
plausible bugs that tests/test_train_ref.py shows every bound can see.

Bounds, as for the LSTM drivers and the CE: allowed = K * E + one rounding of
the storage format, E = max|model - exact|, K = 2. Three bounds are derived
instead: the embedding scatter and the AR/TAR sums from the fp32 summation
bound (n - 1) * 2^-24 * sum|terms|, the AR/TAR backward from counting the
roundings of one element. DropConnect and the embedding gather have exact
references and are compared bit for bit.
"""
import math

import numpy as np
import torch

from ce_ref import half_ulp, vec_of, _rnd
from lstm_ref import FP32_DRIVER_TOL, K_FACTOR

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
K = K_FACTOR["lib_bf16"]        # 2
THREADS = 256                   # every kernel here launches 256-thread blocks
U32 = 2.0 ** -24                # fp32 unit roundoff


def dt_id(dt):
    return "bf16" if dt == BF16 else "fp32"


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ratio(got, exact, allowed):
    """max |got - exact| / allowed. An exact hit counts 0 even where allowed
    is 0; NaN or inf anywhere gives inf."""
    exact = exact.double()
    err = (got.double() - exact).abs()
    allowed = torch.as_tensor(allowed, dtype=F64) + torch.zeros_like(exact)
    r = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


def bound_from_model(model, exact, dtype):
    """K * E + one rounding of ``dtype`` at |exact|, elementwise.

    fp32 tensors of the QRNN scan get the suite's fp32 bound instead,
    FP32_DRIVER_TOL relative to max(1, max|exact|): there the storage
    roundings (E ~ 1e-7) are not the kernel's error, its fast exp is."""
    E = float((model - exact).abs().max())
    return K * E + half_ulp(exact, dtype), E


def fp32_bound(exact):
    return FP32_DRIVER_TOL * max(1.0, float(exact.abs().max())) \
        + torch.zeros_like(exact)


# ---- QRNN fo-pool scan ------------------------------------------------------

QRNN_SHAPES = [(3, 4, 8), (5, 7, 12), (3, 5, 13), (2, 1, 16), (5, 3, 520),
               (3, 3, 101)]
QRNN_KEYS = ("h", "c", "act", "dgates", "dc0")
# wrong variant -> the outputs it must move by 2x the bound
WRONG_QRNN = {
    "fo_swapped": ("h", "act", "dgates"),
    "c0_zero_bwd": ("dgates",),
    "dcT_ignored": ("dgates", "dc0"),
    "last_vec_unwritten": QRNN_KEYS,
    "block_shift": QRNN_KEYS,
}


def qrnn_vec(H, dtype):
    """Columns per thread: the 16-byte vector kernels need H % VEC == 0."""
    v = vec_of(dtype)
    return v if H % v == 0 else 1


def qrnn_wrong_applies(wrong, B, T, H, dtype):
    if wrong == "block_shift":      # needs a second workgroup
        return B * (H // qrnn_vec(H, dtype)) > THREADS
    return True


def qrnn_inputs(B, T, H, dtype, scale=1.0):
    """Pre-activations, c0, dh and dcT of order 1, rounded to ``dtype``."""
    g = _gen(B, T, H, dtype == BF16, int(scale))
    r = lambda *s: torch.randn(*s, generator=g)
    gates = scale * r(B, T, 3 * H)
    if scale != 1.0:
        # saturated: keep the forget gate of the last columns open, or
        # nothing of c0 and dcT would reach c and dc0 there
        gates[..., 2 * H - 8:2 * H].abs_()
    return dict(gates=gates.to(dtype),
                c0=r(B, H).to(dtype), dh=r(B, T, H).to(dtype),
                dcT=r(B, H).to(dtype))


def qrnn_forward(gates, c0, st=None, carry=None):
    """fp64 scan on pre-activations. ``st`` rounds a stored value (act, c,
    h), ``carry`` the running c; None leaves fp64. h is formed from the
    carried c and the unrounded gates, as the kernel does."""
    st = st or (lambda t: t)
    carry = carry or (lambda t: t)
    H = gates.shape[-1] // 3
    z = gates[..., :H].tanh()
    f = gates[..., H:2 * H].sigmoid()
    o = gates[..., 2 * H:].sigmoid()
    c, hs, cs = c0, [], []
    for t in range(gates.shape[1]):
        c = carry(f[:, t] * c + (1 - f[:, t]) * z[:, t])
        cs.append(st(c))
        hs.append(st(o[:, t] * c))
    return (torch.stack(hs, 1), torch.stack(cs, 1),
            st(torch.cat([z, f, o], -1)))


def qrnn_backward(act, c, c0, dh, dcT, st=None, carry=None, wrong=None):
    """Closed-form backward from the ACTIVATED gates and the saved c:
    (dgates w.r.t. the pre-activations, dc0)."""
    st = st or (lambda t: t)
    carry = carry or (lambda t: t)
    H = c0.shape[-1]
    z, f, o = act[..., :H], act[..., H:2 * H], act[..., 2 * H:]
    dc = torch.zeros_like(dcT) if wrong == "dcT_ignored" else dcT
    T = act.shape[1]
    dg = [None] * T
    for t in range(T - 1, -1, -1):
        cprev = c[:, t - 1] if t else \
            (torch.zeros_like(c0) if wrong == "c0_zero_bwd" else c0)
        dc = carry(dc + dh[:, t] * o[:, t])
        dz = dc * (1 - f[:, t]) * (1 - z[:, t] ** 2)
        df = dc * (cprev - z[:, t]) * f[:, t] * (1 - f[:, t])
        do = dh[:, t] * c[:, t] * o[:, t] * (1 - o[:, t])
        dc = carry(dc * f[:, t])
        dg[t] = st(torch.cat([dz, df, do], -1))
    return torch.stack(dg, 1), st(dc)


def _lanes(t, H, vec):
    """(..., B, T, k*H) -> (B * H/vec, T, k, vec): one row per thread."""
    B, T = t.shape[0], t.shape[1]
    k = t.shape[2] // H
    return t.reshape(B, T, k, H // vec, vec).permute(0, 3, 1, 2, 4) \
        .reshape(B * (H // vec), T, k, vec)


def _unlanes(l, B, H, vec):
    T, k = l.shape[1], l.shape[2]
    return l.reshape(B, H // vec, T, k, vec).permute(0, 2, 3, 1, 4) \
        .reshape(B, T, k * H)


def qrnn_exact(inp, wrong=None):
    """All five outputs in fp64; dc0 and c0-shaped tensors are (B, H)."""
    dtype = inp["gates"].dtype
    gates, c0, dh, dcT = (inp[k].double() for k in
                          ("gates", "c0", "dh", "dcT"))
    B, T, H3 = gates.shape
    H = H3 // 3
    if wrong == "fo_swapped":
        z, f, o = gates.split(H, -1)
        gates = torch.cat([z, o, f], -1)
    h, c, act = qrnn_forward(gates, c0)
    dgates, dc0 = qrnn_backward(act, c, c0, dh, dcT, wrong=wrong)
    out = dict(h=h, c=c, act=act, dgates=dgates, dc0=dc0)
    vec = qrnn_vec(H, dtype)
    if wrong == "last_vec_unwritten":
        # never-written outputs: the in-place gates keep the pre-activation,
        # a fresh buffer is taken as zeros
        for k in ("h", "c", "dgates"):
            out[k] = out[k].clone()
            out[k].reshape(B, T, -1, H)[..., H - vec:] = 0
        out["act"] = act.clone()
        out["act"].reshape(B, T, 3, H)[..., H - vec:] = \
            gates.reshape(B, T, 3, H)[..., H - vec:]
        out["dc0"] = dc0.clone()
        out["dc0"][:, H - vec:] = 0
    if wrong == "block_shift":
        # threads of workgroup >= 1 write their neighbour's result
        for k in QRNN_KEYS:
            t = out[k] if out[k].dim() == 3 else out[k][:, None]
            l = _lanes(t, H, vec).clone()
            l[THREADS:] = l[THREADS:].roll(-1, 0)
            t = _unlanes(l, B, H, vec)
            out[k] = t if out[k].dim() == 3 else t[:, 0]
    return out


def qrnn_model(inp):
    """The kernels' storage roundings: c carried in fp32; c and the
    activated gates stored in T; h formed from the unrounded values; the
    backward reads the stored gates and c and carries dc in fp32."""
    dtype = inp["gates"].dtype
    gates, c0, dh, dcT = (inp[k].double() for k in
                          ("gates", "c0", "dh", "dcT"))
    st = lambda t: _rnd(t, dtype)
    carry = lambda t: _rnd(t, F32)
    h, c, act = qrnn_forward(gates, c0, st, carry)
    dgates, dc0 = qrnn_backward(act, c, c0, dh, dcT, st, carry)
    return dict(h=h, c=c, act=act, dgates=dgates, dc0=dc0)


_cache = {}


def _cached(fn):
    def wrapper(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    return wrapper


@_cached
def qrnn_case(B, T, H, dtype, scale=1.0):
    """Inputs, exact outputs, E and the allowed error of one case
    (computed once; read-only)."""
    return qrnn_eval(qrnn_inputs(B, T, H, dtype, scale))


def qrnn_eval(inp):
    """exact, model, E and allowed for given inputs."""
    dtype = inp["gates"].dtype
    exact, model = qrnn_exact(inp), qrnn_model(inp)
    allowed, E = {}, {}
    for k in QRNN_KEYS:
        allowed[k], E[k] = bound_from_model(model[k], exact[k], dtype)
        if dtype == F32:
            allowed[k] = fp32_bound(exact[k])
    return dict(inp=inp, exact=exact, model=model, allowed=allowed, E=E)


def qrnn_cases():
    return [(B, T, H, dt) for (B, T, H) in QRNN_SHAPES for dt in (F32, BF16)]


# pre-activations scaled by 8: f and o saturate to exactly 0 or 1
QRNN_SAT_SHAPE, QRNN_SAT_SCALE = (5, 7, 12), 8.0


def qrnn_scaled_cases():
    """(B, T, H, dtype, scale): every case, plus the saturated ones."""
    return [c + (1.0,) for c in qrnn_cases()] + \
        [QRNN_SAT_SHAPE + (dt, QRNN_SAT_SCALE) for dt in (F32, BF16)]


def qrnn_scaled_id(c):
    return qrnn_case_id(c) + ("-x8" if c[4] != 1.0 else "")


def qrnn_case_id(c):
    return f"{dt_id(c[3])}-B{c[0]}T{c[1]}H{c[2]}"


# ---- fused AdamW ------------------------------------------------------------

ADAM_NS = (1, 255, 256, 257, 1000)
ADAM_BETAS = (0.9, 0.99)
ADAM_LR = 1e-3
WRONG_ADAM = ("l2", "eps_in_sqrt", "bc2_outside", "other_step", "no_master")
ADAM_KEYS = ("master", "exp_avg", "exp_avg_sq")


def adam_cases():
    """(n, dtype, steps, wd, eps). The eps = 1e-3 cases draw gradients
    between 1e-3 and 1, so that where eps sits matters."""
    out = [(n, dt, steps, wd, 1e-8) for dt in (F32, BF16) for n in ADAM_NS
           for steps in (1, 20) for wd in (0.0, 0.1)]
    return out + [(257, dt, 20, 0.1, 1e-3) for dt in (F32, BF16)]


def adam_case_id(c):
    n, dt, steps, wd, eps = c
    return f"{dt_id(dt)}-n{n}-s{steps}-wd{wd}-eps{eps:g}"


def adam_wrong_applies(wrong, case):
    n, dt, steps, wd, eps = case
    if wrong == "l2":
        return wd > 0
    if wrong == "eps_in_sqrt":
        return eps >= 1e-3
    if wrong == "no_master":
        return dt == BF16
    return True


def adam_inputs(n, dtype, steps, eps):
    """p0 with 0.5 <= |p0| < 1.9 (so the decay term is never negligible and
    one step is below half a bf16 ulp) and ``steps`` fresh gradients."""
    g = _gen(n, dtype == BF16, steps, int(eps * 1e9))
    sign = lambda *s: torch.randint(0, 2, s, generator=g) * 2.0 - 1.0
    p0 = (sign(n) * (0.5 + 1.4 * torch.rand(n, generator=g))).to(dtype)
    if eps >= 1e-3:
        grads = [(sign(n) * 10.0 ** (-3.0 * torch.rand(n, generator=g)))
                 .to(dtype) for _ in range(steps)]
    else:
        grads = [torch.randn(n, generator=g).to(dtype) for _ in range(steps)]
    return p0, grads


def _f32(x):
    return float(np.float32(x))


def adam_run(p0, grads, lr, betas, eps, wd, model=False, wrong=None,
             start_step=0):
    """(master, exp_avg, exp_avg_sq) in fp64 after one step per gradient.

    ``model``: the kernel's storage roundings. Its scalar arguments arrive
    as fp32 (lr, betas, eps, wd, both bias corrections) and 1 - lr*wd,
    1 - beta are formed in fp32; master and both moments are rounded to
    fp32 after every step."""
    b1, b2 = betas
    m = p0.double().clone()
    ea, eas = torch.zeros_like(m), torch.zeros_like(m)
    f = np.float32
    for i, g in enumerate(grads):
        step = start_step + i + 1
        bstep = step + 1 if wrong == "other_step" else step
        bc1, bc2 = 1 - b1 ** bstep, 1 - b2 ** bstep
        if model:
            decay = float(f(1) - f(lr) * f(wd))
            c1, c2 = float(f(1) - f(b1)), float(f(1) - f(b2))
            k1, k2, lr_, eps_ = _f32(b1), _f32(b2), _f32(lr), _f32(eps)
            bc1, bc2 = _f32(bc1), _f32(bc2)
        else:
            decay, c1, c2, k1, k2, lr_, eps_ = \
                1 - lr * wd, 1 - b1, 1 - b2, b1, b2, lr, eps
        g = g.double()
        if wrong == "l2":
            g = g + wd * m
        else:
            m = m * decay
        ea = k1 * ea + c1 * g
        eas = k2 * eas + c2 * g * g
        if wrong == "eps_in_sqrt":
            den = (eas / bc2 + eps_).sqrt()
        elif wrong == "bc2_outside":
            den = eas.sqrt() / bc2 + eps_
        else:
            den = (eas / bc2).sqrt() + eps_
        m = m - lr_ * (ea / bc1) / den
        if model:
            m, ea, eas = _rnd(m, F32), _rnd(ea, F32), _rnd(eas, F32)
        if wrong == "no_master":
            m = _rnd(m, BF16)
    return dict(master=m, exp_avg=ea, exp_avg_sq=eas)


@_cached
def _adam_single(n, dtype, steps, wd, eps):
    p0, grads = adam_inputs(n, dtype, steps, eps)
    a = (p0, grads, ADAM_LR, ADAM_BETAS, eps, wd)
    exact, model = adam_run(*a), adam_run(*a, model=True)
    E = {k: float((model[k] - exact[k]).abs().max()) for k in ADAM_KEYS}
    return dict(p0=p0, grads=grads, exact=exact, model=model, E=E)


@_cached
def adam_case(n, dtype, steps, wd, eps):
    """allowed = K * E + half an fp32 ulp. E is the largest over the sizes
    that share (dtype, steps, wd, eps): the values have the same spread at
    every n, and one element (n = 1) says little about how large a rounding
    error gets."""
    c = dict(_adam_single(n, dtype, steps, wd, eps))
    ns = ADAM_NS if eps < 1e-3 else (n,)
    E = {k: max(_adam_single(m, dtype, steps, wd, eps)["E"][k] for m in ns)
         for k in ADAM_KEYS}
    c["E"] = E
    c["allowed"] = {k: K * E[k] + half_ulp(c["exact"][k], F32)
                    for k in ADAM_KEYS}
    return c


@_cached
def two_param_case(dtype):
    """Two parameters over 6 steps; the second has no gradient on odd
    steps (0-based), so it takes 3 steps with its own bias correction.
    ``wrong``: the second parameter corrected with the first one's count."""
    n, steps, wd, eps = 257, 6, 0.1, 1e-8
    pa, ga = adam_inputs(n, dtype, steps, eps)
    pb, gb = adam_inputs(n + 1, dtype, steps, eps)
    grad_steps = [[ga[i], gb[i] if i % 2 == 0 else None]
                  for i in range(steps)]
    a = (ADAM_LR, ADAM_BETAS, eps, wd)
    exact, allowed = [], []
    for p0, gs in ((pa, ga), (pb, gb[0::2])):
        ex = adam_run(p0, gs, *a)["master"]
        E = float((adam_run(p0, gs, *a, model=True)["master"] - ex)
                  .abs().max())
        exact.append(ex)
        allowed.append(K * E + half_ulp(ex, F32))
    # the first parameter's count at the second's k-th step is 2k - 1
    wrong = adam_run_counts(pb, gb[0::2], [1, 3, 5], *a)
    return dict(p0=[pa, pb], grad_steps=grad_steps, exact=exact,
                allowed=allowed, wrong=wrong)


def adam_run_counts(p0, grads, counts, lr, betas, eps, wd):
    """fp64 AdamW whose bias corrections use ``counts`` as step numbers."""
    b1, b2 = betas
    m = p0.double().clone()
    ea, eas = torch.zeros_like(m), torch.zeros_like(m)
    for g, step in zip(grads, counts):
        g = g.double()
        m = m * (1 - lr * wd)
        ea = b1 * ea + (1 - b1) * g
        eas = b2 * eas + (1 - b2) * g * g
        m = m - lr * (ea / (1 - b1 ** step)) / \
            ((eas / (1 - b2 ** step)).sqrt() + eps)
    return m


# sub-ulp accumulation: 64 steps of lr = 1e-4 from p = 1.0 with gradient 1
SUBULP = dict(n=257, lr=1e-4, steps=64, eps=1e-8, wd=0.0)


def subulp_exact():
    p0 = torch.ones(SUBULP["n"], dtype=BF16)
    grads = [torch.ones(SUBULP["n"], dtype=BF16)] * SUBULP["steps"]
    a = (p0, grads, SUBULP["lr"], ADAM_BETAS, SUBULP["eps"], SUBULP["wd"])
    exact, model = adam_run(*a), adam_run(*a, model=True)
    E = float((model["master"] - exact["master"]).abs().max())
    return exact["master"], K * E + half_ulp(exact["master"], F32)


# ---- seeded DropConnect -----------------------------------------------------

DC_NS = (1, 7, 8, 2048, 2049, 4357)
DC_SEEDS = (0, 12345, 2 ** 62 - 1)
DC_PS = (0.2, 0.5)


def dc_keep(p):
    """(keep, thresh, 1/keep) exactly as launch_dc forms them in fp32."""
    f = np.float32
    keep = f(1) - f(p)
    thresh = np.uint32(min(f(keep * f(4294967296.0)), f(4294967295.0)))
    return keep, thresh, f(1) / keep


def dc_mask(n, seed, p):
    """bool[n]: element i is kept. splitmix64 finaliser of seed ^ i, upper
    32 bits against the keep threshold (uint64 arithmetic wraps)."""
    x = np.uint64(seed) ^ np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return torch.from_numpy((x >> np.uint64(32)) < np.uint64(dc_keep(p)[1]))


def dc_apply(v, seed, p):
    """fp32(v) * fp32(1/keep) rounded to v's dtype where kept, +0.0
    elsewhere; any shape, elements numbered in contiguous order."""
    inv = torch.tensor(float(dc_keep(p)[2]), dtype=F32)
    keep = dc_mask(v.numel(), seed, p).reshape(v.shape)
    scaled = (v.float() * inv).to(v.dtype)
    return torch.where(keep, scaled, torch.zeros_like(scaled))


def dc_input(n, dtype):
    """Non-zero values of both signs (so a dropped element is told from a
    kept one)."""
    g = _gen(n, dtype == BF16, 3)
    v = torch.randn(n, generator=g)
    return (v + v.sign() * 0.25).to(dtype)


def bits(t):
    """Integer view for bit-for-bit comparison."""
    return t.contiguous().view(torch.int16 if t.dtype == BF16
                               else torch.int32)


# ---- embedding gather / scatter ---------------------------------------------

EMB_V, EMB_PAD, EMB_P = 11, 1, 0.25
EMB_SHAPES = [((103,), 5), ((2, 4), 64), ((3, 4, 25), 48)]   # ids shape, E
WRONG_SCATTER = ("pad_not_skipped", "mask_not_applied", "dup_overwritten")


EMB_SINGLE_ROW = ((3, 4, 25), 48, F32, True)   # run with all ids on row 3


def emb_cases():
    return [(shape, E, dt, masked) for (shape, E) in EMB_SHAPES
            for dt in (F32, BF16) for masked in (False, True)]


def emb_case_id(c):
    shape, E, dt, masked = c
    return f"{dt_id(dt)}-n{math.prod(shape)}-E{E}-" \
        f"{'mask' if masked else 'nomask'}"


def emb_inputs(shape, E, dtype, masked, single_row=None):
    """ids holding 0, V - 1, the pad row and every row but row 2 many times;
    a row mask of zeros and 1/(1 - p) with rows 0, 1 and V - 1 kept."""
    n = math.prod(shape)
    g = _gen(n, E, dtype == BF16, masked)
    rows = torch.tensor([0, EMB_V - 1, EMB_PAD, 0, 5, EMB_V - 1, EMB_PAD, 7])
    ids = torch.randint(0, EMB_V, (n,), generator=g)
    ids[ids == 2] = 3                       # row 2 is never looked up
    ids[:8] = rows[:n]
    if single_row is not None:
        ids[:] = single_row
    w = torch.randn(EMB_V, E, generator=g).to(dtype)
    gout = (torch.randn(n, E, generator=g) + 0.5).to(dtype)
    mask = torch.empty(0, dtype=F32)
    if masked:
        keep = torch.rand(EMB_V, generator=g) > EMB_P
        keep[[0, EMB_PAD, EMB_V - 1, 5]] = True
        keep[7] = False
        mask = keep.float() / torch.tensor(1 - EMB_P, dtype=F32)
    return dict(ids=ids.reshape(shape), w=w, gout=gout.reshape(*shape, E),
                mask=mask)


def gather_exact(w, ids, mask):
    """round_T(fp32(w[row, e]) * mask[row]): one fp32 product, so the
    kernel must match bit for bit."""
    v = w.float()[ids]
    if mask.numel():
        v = v * mask[ids][..., None]
    return v.to(w.dtype)


def scatter_exact(gout, ids, mask, V, pad, wrong=None):
    """(dW in fp64, allowed). Each thread adds the fp32 product
    fp32(g) * mask[row] atomically; the products are exact to reproduce, the
    order of the additions is not. Summing n terms in fp32 in any order errs
    by at most (n - 1) * 2^-24 * sum|terms| (the first addition, to 0, is
    exact): that is the bound, per element, n = times the row is looked up.
    A row looked up once must therefore be exact."""
    E = gout.shape[-1]
    ids = ids.reshape(-1)
    terms = gout.float().reshape(-1, E)
    if mask.numel() and wrong != "mask_not_applied":
        terms = terms * mask[ids][:, None]
    terms = terms.double()
    live = torch.ones_like(ids, dtype=torch.bool) \
        if wrong == "pad_not_skipped" else ids != pad
    dw = torch.zeros(V, E, dtype=F64)
    mag = torch.zeros(V, E, dtype=F64)
    cnt = torch.zeros(V, dtype=F64)
    if wrong == "dup_overwritten":
        for i in live.nonzero().flatten().tolist():
            dw[ids[i]] = terms[i]
    else:
        dw.index_add_(0, ids[live], terms[live])
    mag.index_add_(0, ids[live], terms[live].abs())
    cnt.index_add_(0, ids[live], torch.ones(int(live.sum()), dtype=F64))
    allowed = (cnt - 1).clamp_min(0)[:, None] * U32 * mag
    return dw, allowed


# ---- AR/TAR -----------------------------------------------------------------

WRONG_ARTAR = ("tail_dropped", "last_row_up", "first_dn_missing",
               "second_trip_skipped", "dloss_ignored")
ARTAR_DLOSS = float(np.float32(1.7))
ARTAR_ALPHA, ARTAR_BETA = 2.0, 1.0

# (name, dtype, n_out, r shape (T, B, H))
ARTAR_CASES = [
    (f"{dt_id(dt)}-{name}", dt, n_out, shape)
    for dt in (F32, BF16)
    for name, n_out, shape in (
        ("tail-T3", 1027, (3, 1, 8)),        # n_out > n_r, tail for both VECs
        ("T2", 1027, (2, 1, 8)),
        ("short-out", 13, (3, 2, 16)),       # n_out < n_r
    )
] + [
    # fp32: 512 blocks * 256 threads * 4 = 524 288 elements per trip. With
    # T = 5 the backward loops take a second trip and its tail; the forward
    # difference loop (n_r - B*H elements) needs T = 6 for one
    ("fp32-second-trip", F32, 524288 + 7, (5, 8, 16384)),
    ("fp32-second-trip-T6", F32, 524288 + 7, (6, 8, 16384)),
]


def artar_geometry(n_out, n_r, dtype):
    """(VEC, blocks, grid stride in elements) as artar_blocks sizes them."""
    vec = vec_of(dtype)
    per = THREADS * 8
    blocks = min(8192, max((max(n_out, n_r) + per - 1) // per, 512))
    return vec, blocks, blocks * THREADS * vec


def artar_coeffs(n_out, shape):
    m = max(shape[1] * (shape[0] - 1) * shape[2], 1)
    return 2.0 * ARTAR_ALPHA / max(n_out, 1), 2.0 * ARTAR_BETA / m


def artar_inputs(dtype, n_out, shape):
    """Order-1 values; large ones in the last n % VEC elements of out and
    in the first and last time row of r."""
    g = _gen(n_out, shape[0], shape[2], dtype == BF16)
    out = torch.randn(n_out, generator=g)
    out[-(n_out % 8 or 1):] *= 30.0
    r = torch.randn(*shape, generator=g)
    r[0] *= 4.0
    r[-1] *= 4.0
    return out.to(dtype), r.to(dtype)


def artar_exact(out, r_tm, g, ca, cb, wrong=None):
    """fp64 sums [sum out^2, sum (r[t+1] - r[t])^2] and both gradients, with
    the magnitudes the backward bound needs."""
    dtype = out.dtype
    o = out.double().reshape(-1)
    T = r_tm.shape[0]
    rf = r_tm.double().reshape(T, -1)
    n_out = o.numel()
    vec, blocks, stride = artar_geometry(n_out, rf.numel(), dtype)
    live = torch.ones(n_out, dtype=torch.bool)
    if wrong == "tail_dropped":
        live[n_out - n_out % vec:] = False
    if wrong == "second_trip_skipped":
        live[stride:] = False
    d = (rf[1:] - rf[:-1]).reshape(-1)
    if wrong == "second_trip_skipped":
        d = d[:stride]
    sq, df = (o[live] ** 2).sum(), (d ** 2).sum()
    if wrong == "last_row_up":
        df = df + ((rf[0] - rf[-1]) ** 2).sum()
    gg = 1.0 if wrong == "dloss_ignored" else g
    dout = ca * gg * o * live
    up, dn = torch.zeros_like(rf), torch.zeros_like(rf)
    up[:-1] = rf[1:]
    dn[1:] = rf[:-1]
    s = torch.zeros_like(rf)
    s[:-1] += rf[:-1] - rf[1:]
    s[1:] += rf[1:] - rf[:-1]
    if wrong == "last_row_up":
        s[-1] += rf[-1] - rf[0]
    if wrong == "first_dn_missing":
        s[1] -= rf[1] - rf[0]
    dr = cb * gg * s
    if wrong == "second_trip_skipped":
        dr.reshape(-1)[stride:] = 0
    dr_mag = abs(cb * g) * (2 * rf.abs() + up.abs() + dn.abs())
    return dict(sq=sq, df=df, dout=dout.reshape(out.shape),
                dr=dr.reshape(r_tm.shape), dr_mag=dr_mag.reshape(r_tm.shape))


def artar_sum_bound(n, n_out, n_r, dtype):
    """Relative bound of one of the forward sums over n elements.

    Every term is >= 0, so the fp32 summation bound (chain - 1) * 2^-24 *
    sum|terms| is relative to the sum. The longest chain of additions one
    term goes through: the terms of one thread (grid-stride trips * VEC),
    6 shuffle steps, 4 waves, and one atomic add per block. Each term's own
    arithmetic adds 3 more roundings: its product, and for the difference
    of two fp32 values one rounding that the square doubles."""
    vec, blocks, stride = artar_geometry(n_out, n_r, dtype)
    trips = max(1, -(-n // stride))
    return (trips * vec + 6 + 4 + blocks + 3) * U32


def artar_grad_bounds(ex, ca, g, dtype):
    """Elementwise: 4 fp32 ulps of |ca*g*o|, respectively of
    |cb*g| * (2|a| + |up| + |dn|), plus half an ulp of T: the coefficient
    arrives rounded to fp32, and the products and the two differences each
    round once."""
    ulp4 = 4 * 2.0 ** -23
    return (ulp4 * ex["dout"].abs() + half_ulp(ex["dout"], dtype),
            ulp4 * ex["dr_mag"] + half_ulp(ex["dr"], dtype))


@_cached
def artar_case(name):
    name, dtype, n_out, shape = next(c for c in ARTAR_CASES if c[0] == name)
    out, r = artar_inputs(dtype, n_out, shape)
    ca, cb = artar_coeffs(n_out, shape)
    ex = artar_exact(out, r, ARTAR_DLOSS, ca, cb)
    n_r = r.numel()
    rel = dict(sq=artar_sum_bound(n_out, n_out, n_r, dtype),
               df=artar_sum_bound(n_r - shape[1] * shape[2], n_out, n_r,
                                  dtype))
    a_dout, a_dr = artar_grad_bounds(ex, ca, ARTAR_DLOSS, dtype)
    allowed = dict(sq=rel["sq"] * ex["sq"], df=rel["df"] * ex["df"],
                   dout=a_dout, dr=a_dr)
    return dict(out=out, r=r, ca=ca, cb=cb, exact=ex, allowed=allowed,
                dtype=dtype)


def artar_wrong_applies(wrong, dtype, n_out, shape):
    n_r = math.prod(shape)
    vec, blocks, stride = artar_geometry(n_out, n_r, dtype)
    if wrong == "tail_dropped":
        return n_out % vec != 0
    if wrong == "second_trip_skipped":
        return max(n_out, n_r) > stride
    return True


def artar_shows(wrong, dtype, n_out, shape):
    """The outputs a wrong variant must move by 2x the bound."""
    if wrong == "second_trip_skipped":
        n_r, BH = math.prod(shape), shape[1] * shape[2]
        stride = artar_geometry(n_out, n_r, dtype)[2]
        return tuple(k for k, n in (("sq", n_out), ("dout", n_out),
                                    ("df", n_r - BH), ("dr", n_r))
                     if n > stride)
    return {"tail_dropped": ("sq", "dout"), "last_row_up": ("df", "dr"),
            "first_dn_missing": ("dr",),
            "dloss_ignored": ("dout", "dr")}[wrong]

# bf16 needs more than 8192 * 256 * 8 = 16 777 216 elements for a second
# grid-stride trip: artar_blocks caps the grid at 8192 blocks
# (T = 10 so that the forward difference loop, n_r - B*H elements, is past it
# as well)
ARTAR_BIG_R = (10, 8, 262144)
ARTAR_BIG_OUT = 16777216 + 8 + 3


@_cached
def artar_big_case():
    """bf16 inputs just past the second trip, built by tiling a small random
    block; distinct large values where only the second trip reads. Exact
    sums over everything, gradients on windows at the start, around the
    stride boundary, the time-row boundaries and the end."""
    g = _gen(77)
    BH = ARTAR_BIG_R[1] * ARTAR_BIG_R[2]
    n_r = ARTAR_BIG_R[0] * BH
    vec, blocks, stride = artar_geometry(ARTAR_BIG_OUT, n_r, BF16)
    assert stride == 16777216 and n_r - BH > stride
    blk = torch.randn(6151, generator=g)

    def tiled(n, base):
        t = blk.repeat(-(-n // blk.numel()))[:n].clone()
        t[stride:] = base + torch.arange(n - stride).remainder(509) / 16.0
        return t.to(BF16)

    # out has 11 elements past the stride: large enough to outweigh the
    # summation bound of the 16.7M before them
    out, r = tiled(ARTAR_BIG_OUT, 64.0), tiled(n_r, 8.0).reshape(ARTAR_BIG_R)
    ca, cb = artar_coeffs(ARTAR_BIG_OUT, ARTAR_BIG_R)
    rf = r.reshape(-1)

    def chunks(n, step=1 << 22):
        return [(s, min(n, s + step)) for s in range(0, n, step)]

    sq = sum(float((out[a:b].double() ** 2).sum())
             for a, b in chunks(ARTAR_BIG_OUT))
    df = sum(float(((rf[a + BH:b + BH].double() - rf[a:b].double()) ** 2)
                   .sum()) for a, b in chunks(n_r - BH))
    sq2 = float((out[stride:].double() ** 2).sum())
    df2 = float(((rf[stride + BH:].double() - rf[stride:n_r - BH].double())
                 ** 2).sum())
    W = 4096
    wins_r = [(max(0, c - W), min(n_r, c + W))
              for c in (0, BH, stride, 2 * BH, n_r)]
    wins_o = [(max(0, c - W), min(ARTAR_BIG_OUT, c + W))
              for c in (0, stride, ARTAR_BIG_OUT)]
    gg = ARTAR_DLOSS
    ulp4 = 4 * 2.0 ** -23
    dr = {}
    for a, b in wins_r:
        i = torch.arange(a, b)
        x = rf[a:b].double()
        up = torch.where(i + BH < n_r, rf[(i + BH).clamp_max(n_r - 1)]
                         .double(), torch.zeros_like(x))
        dn = torch.where(i >= BH, rf[(i - BH).clamp_min(0)].double(),
                         torch.zeros_like(x))
        s = (x - up) * (i + BH < n_r) + (x - dn) * (i >= BH)
        e = cb * gg * s
        mag = abs(cb * gg) * (2 * x.abs() + up.abs() + dn.abs())
        dr[(a, b)] = (e, ulp4 * mag + half_ulp(e, BF16))
    dout = {}
    for a, b in wins_o:
        e = ca * gg * out[a:b].double()
        dout[(a, b)] = (e, ulp4 * e.abs() + half_ulp(e, BF16))
    rel = dict(sq=artar_sum_bound(ARTAR_BIG_OUT, ARTAR_BIG_OUT, n_r, BF16),
               df=artar_sum_bound(n_r - BH, ARTAR_BIG_OUT, n_r, BF16))
    return dict(out=out, r=r, ca=ca, cb=cb, sq=sq, df=df, sq2=sq2, df2=df2,
                rel=rel, dr=dr, dout=dout, stride=stride)
