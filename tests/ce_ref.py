"""fp64 references for the tied-decoder CE path (plain torch, no project
code): the epilogue kernels of ce.hip, the quantize kernel of fp8util.hip
and ``tied_decoder_ce`` end to end.

``epilogue_exact`` / ``ce_exact`` are the mathematical operation in fp64.
``ce_model`` is the same arithmetic with the roundings each path performs
when it stores a value (e4m3 inputs, bf16/fp32 logits and dlogits, e4m3
dlogits copy), still evaluated in fp64 in between. The distance between
the two is the error a correct kernel is entitled to; the tests derive
their bounds from it and from the storage formats, never from the kernels.

Every function also takes ``wrong=<name>`` (see WRONG_*): deliberately
broken variants of the arithmetic, used by tests/test_ce_ref.py to show
that each bound is at least 2x below what such an error would cause.
"""
import math

import torch

from lstm_ref import FP32_DRIVER_TOL, K_FACTOR

BF16, F32, F8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
STORE = 448.0                   # e4m3 dlogits store scale, also e4m3 max
K = K_FACTOR["lib_bf16"]        # 2, as for the LSTM drivers


def vec_of(dtype):
    """Elements per 16-byte vector: the kernels' VEC."""
    return 4 if dtype == F32 else 8


def _rnd(t, dtype):
    """Round an fp64 tensor through a storage type."""
    return t.to(dtype).double()


def _binade(x):
    """floor(log2|x|) elementwise (exact, via frexp); 0 maps to -inf."""
    m, e = torch.frexp(x.abs().double())
    e = e.double() - 1
    return torch.where(x == 0, torch.full_like(e, -math.inf), e)


def half_ulp(x, dtype):
    """Half a unit in the last place of ``dtype`` at |x| (fp64 tensor):
    the rounding error of one correctly rounded store of x."""
    mant = {BF16: 7, F32: 23}[dtype]
    return torch.exp2(_binade(x) - mant - 1)


def e4m3_half_step(x):
    """Half the spacing of e4m3 values around |x|: 3 mantissa bits, normal
    binades down to 2^-6, below that the subnormal step 2^-9 (so anything
    under 2^-10 may flush to zero)."""
    return torch.exp2(_binade(x).clamp_min(-6.0) - 3 - 1)


# ---- quantize_e4m3 ---------------------------------------------------------

def quantize_exact(x, scale):
    """clamp(x / scale, +-448) cast to e4m3 with the fp32 division. The
    division is correctly rounded, so a kernel must match byte for byte
    (NaN stays NaN: clamp propagates it and the cast gives the NaN code)."""
    s = torch.as_tensor(scale, dtype=F32)
    return (x.float() / s).clamp(-STORE, STORE).to(F8)


def quantize_by_reciprocal(x, scale):
    """The WRONG rule: x * (1/scale), two fp32 roundings instead of one."""
    s = torch.as_tensor(scale, dtype=F32)
    return (x.float() * (1.0 / s)).clamp(-STORE, STORE).to(F8)


# With scale 7, fp32(1/7) is 2.1e-8 (relative) too large: for these inputs
# x / 7 is EXACTLY the midpoint of two adjacent e4m3 values (a tie, rounds
# to even) and x * fp32(1/7) rounds to the next fp32 above the midpoint, so
# it rounds away. All are bf16-representable (at most 8 significant bits).
TIE_SCALE = 7.0


def tie_inputs():
    """All positive bf16-representable x with x / TIE_SCALE an exact e4m3
    tie on which the reciprocal rule gives the other code (found by search
    on the CPU, asserted non-empty by the CPU test)."""
    codes = torch.arange(0, 0x7f, dtype=torch.uint8).view(F8).double()
    mids = (codes[:-1] + codes[1:]) / 2
    x = mids * TIE_SCALE
    ok = x.to(BF16).double() == x
    x = x[ok].float()
    a = quantize_exact(x, TIE_SCALE).view(torch.uint8)
    b = quantize_by_reciprocal(x, TIE_SCALE).view(torch.uint8)
    return x[a != b]


QUANT_SIZES = (1, 7, 8, 2048, 2048 * 3 + 8 + 3)


def quantize_input(n, dtype):
    """n values for the quantize test at scale TIE_SCALE: ordinary values,
    zeros, e4m3-subnormal quotients, both signs past saturation, a NaN,
    and the tie inputs placed in the first vector, in a later block's
    vector body and in the last n % VEC elements (the scalar tail)."""
    g = torch.Generator().manual_seed(100 + n)
    x = (torch.randn(n, generator=g) * 300).to(dtype).float()
    ties = tie_inputs()
    special = torch.cat([
        torch.tensor([0.0, -0.0, 4000.0, -4000.0, 3136.0, -3137.0]),
        # quotients 2^-7, 3*2^-9, 2^-10 (tie to zero), 2^-9, 0.9*2^-10
        torch.tensor([2.0 ** -7, 3 * 2.0 ** -9, 2.0 ** -10, -2.0 ** -9,
                      0.9 * 2.0 ** -10]) * TIE_SCALE,
        torch.tensor([float("nan")])]).to(dtype).float()
    vec = vec_of(dtype)
    if n >= 2048:
        x[16:16 + special.numel()] = special
        x[n // 2:n // 2 + ties.numel()] = ties         # vector body
    k = min(n, vec)
    x[:k] = ties[:k]                                   # first vector
    tail = n % vec
    if tail:
        # the same tie values again in the scalar tail, and with their
        # signs flipped just before it (body) when there is room
        x[n - tail:] = ties[:tail]
        if n - tail >= tail:
            x[n - 2 * tail:n - tail] = -ties[:tail]
    return x.to(dtype)


# ---- epilogue kernels ------------------------------------------------------

WRONG_EPILOGUE = ("bias_dropped", "bias_twice", "onehot_plus", "onehot_minus",
                  "tail_dropped", "tail_max_ignored", "scale_missing",
                  "store_missing", "scale_twice")


def wrong_applies(wrong, has_bias, V, vec):
    """A variant is only a different computation where its ingredient
    exists: bias variants need a bias, tail variants a scalar tail."""
    if wrong in ("bias_dropped", "bias_twice"):
        return has_bias
    if wrong == "tail_dropped":
        return V % vec != 0
    if wrong == "tail_max_ignored":     # an empty body has nothing to rescale
        return V % vec != 0 and V > vec
    return True


def epilogue_exact(logits, bias, targets, scale, wrong=None, vec=8):
    """fp64 epilogue of logits already holding bf16- or fp32-representable
    values: lse = logsumexp(x + b), tgt = x[t] + b[t], p = exp(x + b - lse),
    q = (p - onehot) * scale (the in-place dlogits), q8 = (p - onehot) * 448
    (what the e4m3 copy encodes). ``vec`` only matters to the tail variants.

    Wrong variants: bias_dropped / bias_twice; onehot_plus / onehot_minus
    (the onehot one column off); tail_dropped (the last V % vec columns
    left out of the row sum); tail_max_ignored (the tail raises the running
    maximum without rescaling the sum gathered so far, so lse is wrong
    whenever the row maximum sits in the tail); scale_missing; store_missing
    (no 448 on the e4m3 copy); scale_twice (the 1/N factor applied twice)."""
    x = logits.double()
    N, V = x.shape
    b = torch.zeros(V, dtype=torch.float64) if bias is None else bias.double()
    if wrong == "bias_dropped":
        b = torch.zeros_like(b)
    elif wrong == "bias_twice":
        b = 2 * b
    z = x + b
    Vv = V // vec * vec
    if wrong == "tail_dropped":
        lse = torch.logsumexp(z[:, :Vv], dim=1)
    elif wrong == "tail_max_ignored":
        m_body = z[:, :Vv].amax(dim=1)
        m_all = z.amax(dim=1)
        body = torch.exp(z[:, :Vv] - m_body[:, None]).sum(dim=1)
        tail = torch.exp(z[:, Vv:] - m_all[:, None]).sum(dim=1)
        lse = m_all + torch.log(body + tail)
    else:
        lse = torch.logsumexp(z, dim=1)
    t = targets.long()
    tgt = z.gather(1, t[:, None]).squeeze(1)
    p = torch.exp(z - lse[:, None])
    hot = t
    if wrong == "onehot_plus":
        hot = (t + 1) % V
    elif wrong == "onehot_minus":
        hot = (t - 1) % V
    pm = p.clone()
    pm[torch.arange(N), hot] -= 1.0
    sc = float(scale)
    if wrong == "scale_missing":
        sc = 1.0
    elif wrong == "scale_twice":
        sc = sc * sc
    return dict(lse=lse, tgt=tgt, p=p, q=pm * sc,
                q8=pm * (1.0 if wrong == "store_missing" else STORE))


def epilogue_allowed(exact, dtype, scale):
    """Per-element error a correct kernel is entitled to, per output.

    lse, tgt: the suite's fp32 bound FP32_DRIVER_TOL, absolute.
    q (fp32 logits): scale * FP32_DRIVER_TOL * p, a RELATIVE bound on p that
      covers the fast exp/log intrinsics and the fp32 row sum (derived for
      these shapes: about 1e-5, see FP32_INTRINSIC_REL), plus one fp32
      rounding of q.
    q (bf16 logits): the same plus half a bf16 ulp of q (2^-9 |q| at the top
      of a binade, 2^-8 |q| at its bottom: computed at q, not assumed).
    q8: the decoded e4m3 value lies within half an e4m3 step of q8 (step
      taken at q8; 2^-9 in the subnormal range, so values under 2^-10 may
      flush to zero) plus 448 * FP32_DRIVER_TOL * p."""
    p, q, q8 = exact["p"], exact["q"], exact["q8"]
    aq = abs(float(scale)) * FP32_DRIVER_TOL * p + half_ulp(q, F32)
    if dtype == BF16:
        aq = aq + half_ulp(q, BF16)
    return dict(lse=torch.full_like(exact["lse"], FP32_DRIVER_TOL),
                tgt=torch.full_like(exact["tgt"], FP32_DRIVER_TOL),
                q=aq,
                q8=e4m3_half_step(q8) + STORE * FP32_DRIVER_TOL * p)


EPILOGUE_ROWS = 3
# dloss = 0.5, N = 3 (not 1), as the fp32 number the kernels are handed
EPILOGUE_SCALE = float(torch.tensor(0.5 / EPILOGUE_ROWS, dtype=F32))
# bf16 (VEC 8): one vector per thread / a second vector for some threads /
# a scalar tail / most threads idle / narrower than one vector.
# fp32 (VEC 4): the same four situations, and 3 < VEC.
EPILOGUE_WIDTHS = {BF16: (2048, 2056, 2051, 40, 5), F32: (1024, 1028, 1027, 3)}


def epilogue_cases():
    """(dtype, V, has_bias, kind, tset). kind: plain / shift80 (logits + 80:
    exp overflows without the max subtraction) / peaked (spread 30: many
    p * 448 in the e4m3 subnormal and flush range). tset picks the targets:
    0 -> columns (0, last of the last full vector, V-1),
    1 -> (first tail column, V-1, 0)."""
    out = []
    for dt in (BF16, F32):
        for V in EPILOGUE_WIDTHS[dt]:
            for has_bias in (False, True):
                for tset in (0, 1):
                    out.append((dt, V, has_bias, "plain", tset))
        tail_w = EPILOGUE_WIDTHS[dt][2]
        out.append((dt, tail_w, True, "shift80", 0))
        out.append((dt, tail_w, True, "peaked", 1))
    return out


def epilogue_case_id(case):
    dt, V, has_bias, kind, tset = case
    return f"{'bf16' if dt == BF16 else 'fp32'}-V{V}-" \
           f"{'bias' if has_bias else 'nobias'}-{kind}-t{tset}"


_ep_cache = {}


def epilogue_case(case):
    """Inputs, fp64 exact outputs and allowed errors of one epilogue case;
    computed once and shared (treat as read-only)."""
    if case in _ep_cache:
        return _ep_cache[case]
    dt, V, has_bias, kind, tset = case
    vec = vec_of(dt)
    Vv = V // vec * vec
    g = torch.Generator().manual_seed(7 * V + 3 * tset + (dt == F32))
    if kind == "peaked":
        x = -30.0 * torch.rand(EPILOGUE_ROWS, V, generator=g)
    else:
        x = 3.0 * torch.randn(EPILOGUE_ROWS, V, generator=g)
    if kind == "shift80":
        x = x + 80.0
    # row 1: the row maximum sits in the last column (a tail column when
    # there is a tail), 2 above everything else
    x[1, V - 1] = x[1].max() + 2.0
    x = x.to(dt)
    bias = 0.5 * torch.randn(V, generator=g) if has_bias else None
    last_vec = Vv - 1 if Vv else 1
    tail_col = Vv if Vv < V else V - 2
    tg = (0, last_vec, V - 1) if tset == 0 else (tail_col, V - 1, 0)
    targets = torch.tensor(tg, dtype=torch.int64)
    exact = epilogue_exact(x, bias, targets, EPILOGUE_SCALE, vec=vec)
    allowed = epilogue_allowed(exact, dt, EPILOGUE_SCALE)
    c = dict(logits=x, bias=bias, targets=targets, scale=EPILOGUE_SCALE,
             exact=exact, allowed=allowed, vec=vec)
    _ep_cache[case] = c
    return c


def worst_ratio(got, exact, allowed):
    """max |got - exact| / allowed; NaN or inf anywhere gives inf."""
    r = (got.double() - exact).abs() / allowed
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    return float(r.max()) if r.numel() else 0.0


# ---- tied_decoder_ce end to end --------------------------------------------

PATHS = ("bf16", "fp32", "fp8_onepass", "fp8_two_kernel", "fp8_tail",
         "fp8_recompute")
WRONG_E2E = ("bias_dropped", "bias_twice", "onehot_plus", "onehot_minus",
             "scale_missing", "store_missing", "scale_twice")


def ce_exact(h, w, b, t):
    """fp64 mean cross-entropy of the tied decoder, differentiable."""
    z = h.double() @ w.double().t()
    if b is not None:
        z = z + b.double()
    return (torch.logsumexp(z, dim=1)
            - z.gather(1, t.long()[:, None]).squeeze(1)).mean()


def ce_exact_grads(h, w, b, t, dloss=1.0, wrong=None, fp8_dh=False):
    """Closed-form fp64 (loss, dh, dW, db) for upstream gradient ``dloss``;
    test_ce_ref.py checks it against autograd through ``ce_exact``.

    Wrong variants as in ``epilogue_exact`` where they apply end to end
    (V = 2064 has no scalar tail); scale_missing drops dloss/N,
    scale_twice applies 1/N twice (the one-pass path stores 1/N and applies
    dloss later: mixing the two up), store_missing loses the 448 between
    the e4m3 copy and dh (only paths whose dh reads that copy: fp8_dh)."""
    hd, wd = h.double(), w.double()
    N, V = hd.shape[0], wd.shape[0]
    bd = torch.zeros(V, dtype=torch.float64) if b is None else b.double()
    if wrong == "bias_dropped":
        bd = torch.zeros_like(bd)
    elif wrong == "bias_twice":
        bd = 2 * bd
    z = hd @ wd.t() + bd
    lse = torch.logsumexp(z, dim=1)
    tl = t.long()
    loss = (lse - z.gather(1, tl[:, None]).squeeze(1)).mean()
    hot = tl
    if wrong == "onehot_plus":
        hot = (tl + 1) % V
    elif wrong == "onehot_minus":
        hot = (tl - 1) % V
    pm = torch.exp(z - lse[:, None])
    pm[torch.arange(N), hot] -= 1.0
    sc = dloss / N
    if wrong == "scale_missing":
        sc = 1.0
    elif wrong == "scale_twice":
        sc = sc / N
    g = pm * sc
    dh = g @ wd
    if wrong == "store_missing" and fp8_dh:
        dh = dh / STORE
    return dict(loss=loss, dh=dh, dW=g.t() @ hd,
                db=None if b is None else g.sum(dim=0))


def _fp8_chunk(c, H, V):
    """The condition under which a chunk of c rows takes the fp8 GEMMs."""
    return c % 16 == 0 and H % 16 == 0 and V % 16 == 0


def ce_model(h, w, b, t, path, dloss=1.0, chunk=None):
    """fp64 arithmetic with the storage roundings of ``path``. Inputs must
    already hold values representable in the path's dtype. Returns
    (loss, dh, dW, db) like ``ce_exact_grads``.

    Modelled: per-tensor e4m3 inputs with amax/448 scales (fp8 paths, on
    chunks whose row count, H and V are multiples of 16; other chunks use
    the bf16 GEMM); logits stored in the activation dtype; lse in fp32; the
    target logit read back from the stored logits (bf16/fp32 paths) or
    recomputed as a gather-dot of bf16-rounded products summed in fp32 (fp8
    paths); dlogits stored as bf16/fp32 and as e4m3 * 448; dh from the e4m3
    copy times the e4m3 weight where the chunk is an fp8 chunk; dW / db
    partial sums stored per chunk in the activation dtype, accumulated in
    fp32 and cast to the weight / bias dtype; on the one-pass path 1/N is
    what the stored dlogits carry and dloss multiplies the fp32 sums."""
    assert path in PATHS, path
    dt = F32 if path == "fp32" else BF16
    fp8 = path.startswith("fp8")
    onepass = path == "fp8_onepass"
    hd, wd = h.double(), w.double()
    N, H = hd.shape
    V = wd.shape[0]
    C = chunk or N
    bd = torch.zeros(V, dtype=torch.float64) if b is None \
        else b.float().double()
    tl = t.long()
    rows = torch.arange(N)
    chunks = [(s, min(N, s + C)) for s in range(0, N, C)]
    if fp8:
        sa = (h.abs().amax().float() / STORE).clamp_min(1e-12)
        sw = (w.abs().amax().float() / STORE).clamp_min(1e-12)
        h8 = quantize_exact(h, sa).double()
        w8 = quantize_exact(w, sw).double()
        sab = sa.double() * sw.double()
    logits = torch.empty(N, V, dtype=torch.float64)
    for s, e in chunks:
        if fp8 and _fp8_chunk(e - s, H, V):
            logits[s:e] = _rnd((h8[s:e] @ w8.t()) * sab, dt)
        else:
            logits[s:e] = _rnd(hd[s:e] @ wd.t(), dt)
    z = logits + bd
    lse = _rnd(torch.logsumexp(z, dim=1), F32)
    if fp8:
        tgt = _rnd(_rnd(_rnd(hd * wd[tl], dt).sum(dim=1), F32) + bd[tl], F32)
    else:
        tgt = _rnd(z[rows, tl], F32)
    loss = _rnd((lse - tgt).mean(), F32)

    pm = torch.exp(z - lse[:, None])
    pm[rows, tl] -= 1.0
    sc = _rnd(torch.tensor((1.0 if onepass else dloss) / N,
                           dtype=torch.float64), F32)
    dlog = _rnd(_rnd(pm, F32) * sc, dt)
    if fp8:
        dlog8 = _rnd(_rnd(pm, F32) * STORE, F32).float() \
            .clamp(-STORE, STORE).to(F8).double()
        s_dh = _rnd(_rnd(torch.tensor(dloss / N, dtype=torch.float64), F32)
                    / STORE, F32) * sw.double()
    dh = torch.empty(N, H, dtype=torch.float64)
    dW = torch.zeros(V, H, dtype=torch.float64)
    db = torch.zeros(V, dtype=torch.float64)
    for s, e in chunks:
        if fp8 and _fp8_chunk(e - s, H, V):
            dh[s:e] = _rnd((dlog8[s:e] @ w8) * s_dh, dt)
        else:
            dh[s:e] = _rnd(dlog[s:e] @ wd, dt)
        dW = _rnd(dW + _rnd(dlog[s:e].t() @ hd[s:e], dt), F32)
        db = _rnd(db + _rnd(dlog[s:e].sum(dim=0), dt), F32)
    if onepass:
        dW, db = dW * dloss, _rnd(db * dloss, F32)
    return dict(loss=loss, dh=dh, dW=_rnd(dW, w.dtype),
                db=None if b is None else _rnd(db, b.dtype),
                dlog=dlog)


# Relative error of p = exp(x + b - lse) as the kernels compute it in fp32,
# beyond the roundings ce_model applies:
#  * __expf(a) = exp2(a * log2(e)): the fp32 product carries a relative
#    2^-24 on an exponent of size 1.44 |a|, i.e. a relative |a| 2^-24 on the
#    result, plus 1 ulp (2^-23) of the hardware exp2. |a| <= 104 (below,
#    fp32 exp underflows): (104 + 2) 2^-24 = 6.3e-6;
#  * the row sum: a thread adds 8 * ceil(V / 2048) <= 16 terms in sequence,
#    then 6 shuffle steps and 4 waves: <= 26 fp32 roundings, 1.6e-6;
#  * __logf = log2 * ln 2 with 1 ulp of log2: < 1e-6 absolute on lse for
#    lse - max <= 8.
# Sum 8.9e-6, rounded up. As an absolute error of lse it is the same figure
# (d lse = d sum / sum).
FP32_INTRINSIC_REL = 1e-5
EPS32 = 2.0 ** -24              # fp32 unit roundoff


def ce_floor(h, w, b, t, dloss, dtype):
    """Per-element floor of the end-to-end bounds: what a correct fp32
    evaluation may add on top of the storage roundings in ``ce_model``.
    It only matters on the fp32 path, where E is about 1e-7.

    half an ulp of the output dtype at the output's magnitude, plus
     * the intrinsics (FP32_INTRINSIC_REL, relative on p, absolute on lse),
     * fp32 accumulation in the GEMMs, by the standard bound: a dot
       product of n terms is off by at most n 2^-24 sum|a_i b_i|. The
       logits (n = H) move lse and the target logit by that much and p
       relatively by twice that; dh sums V terms, dW and db N terms."""
    hd, wd = h.double(), w.double()
    N, H = hd.shape
    V = wd.shape[0]
    ex = ce_exact_grads(h, w, b, t, dloss)
    bd = torch.zeros(V, dtype=torch.float64) if b is None else b.double()
    z = hd @ wd.t() + bd
    p = torch.softmax(z, dim=1)
    A = p.clone()
    A[torch.arange(N), t.long()] -= 1.0
    A = A.abs()
    g = abs(dloss) / N
    zacc = H * EPS32 * (hd.abs() @ wd.abs().t())            # (N, V)
    rel = FP32_INTRINSIC_REL + 2 * zacc.amax(dim=1)         # (N,) on p
    lse_err = FP32_INTRINSIC_REL + (p * zacc).sum(dim=1) \
        + zacc[torch.arange(N), t.long()]
    rp = rel[:, None] * p
    fl = dict(
        loss=half_ulp(ex["loss"], F32) + lse_err.mean(),
        dh=half_ulp(ex["dh"], dtype)
        + g * (rp @ wd.abs() + V * EPS32 * (A @ wd.abs())),
        dW=half_ulp(ex["dW"], w.dtype)
        + g * (rp.t() @ hd.abs() + N * EPS32 * (A.t() @ hd.abs())))
    if b is not None:
        fl["db"] = half_ulp(ex["db"], b.dtype) \
            + g * (rp.sum(dim=0) + N * EPS32 * A.sum(dim=0))
    return fl


def db_sum_bound(model, b_dtype, n_chunks, dloss):
    """Bound on |db.sum()|, whose exact value is 0 (every softmax row sums
    to one). Worst case of every rounding between p and db, from the
    model's stored values: half an ulp per stored dlogit, per element of
    each chunk's partial sum (at most the final magnitude) and of the final
    cast, plus FP32_DRIVER_TOL (relative on p) * dloss for the rows' sums.
    A softmax taken against a foreign lse misses this by its row-sum
    error times dloss."""
    dlog, db = model["dlog"], model["db"]
    dt = BF16 if b_dtype == BF16 else F32
    return float(half_ulp(dlog, dt).sum()
                 + (n_chunks + 1) * half_ulp(db, b_dtype).sum()
                 + FP32_DRIVER_TOL * abs(dloss))


E2E_N, E2E_H, E2E_V = 48, 32, 2064
# Input scales: h 0.5, w 0.2, b 0.1 (logit spread 0.6: every p is of order
# 1/V, so each wrong variant moves the gradients by far more than the fp8
# input error E); "big" multiplies h by 4 and w by 2 (logits of order ten),
# where a softmax against a foreign lse stops summing to one.
SCALES = {"default": (0.5, 0.2, 0.1), "big": (2.0, 0.4, 0.1)}


def e2e_cases():
    """dict(path, N, chunk, save, bias, dloss, scale) for every end-to-end
    run. chunk is CI_CE_CHUNK (16 with dloss 1, 32 with dloss 0.5); save is
    CI_CE_SAVE_LOGITS."""
    out = []

    def add(path, N=E2E_N, chunk=None, save=1, scale="default"):
        for bias in (True, False):
            for dloss in (1.0, 0.5):
                out.append(dict(path=path, N=N, save=save, bias=bias,
                                dloss=dloss, scale=scale,
                                chunk=chunk or (16 if dloss == 1.0 else 32)))
    for path in ("fp32", "bf16"):
        add(path, save=1)
        add(path, save=0)
        add(path, N=23, chunk=7, save=0)
    add("fp8_onepass")
    add("fp8_two_kernel")
    add("fp8_tail", N=E2E_N + 9)
    add("fp8_recompute", save=0)
    add("fp8_recompute", save=0, scale="big")
    return out


def e2e_case_id(c):
    return "-".join([c["path"], f"N{c['N']}", f"c{c['chunk']}",
                     f"save{c['save']}", "bias" if c["bias"] else "nobias",
                     f"dloss{c['dloss']}", c["scale"]])


_e2e_cache = {}


def e2e_case(c):
    """Inputs (rounded to the path's dtype), fp64 exact outputs, the model,
    E and the allowed error per output; computed once and shared."""
    key = e2e_case_id(c)
    if key in _e2e_cache:
        return _e2e_cache[key]
    dt = F32 if c["path"] == "fp32" else BF16
    N, H, V = c["N"], E2E_H, E2E_V
    sh, sw, sb = SCALES[c["scale"]]
    g = torch.Generator().manual_seed(11 + N)
    h = (sh * torch.randn(N, H, generator=g)).to(dt)
    w = (sw * torch.randn(V, H, generator=g)).to(dt)
    b = (sb * torch.randn(V, generator=g)).to(dt) if c["bias"] else None
    t = torch.randint(0, V, (N,), generator=g)
    t[0], t[1] = 0, V - 1
    exact = ce_exact_grads(h, w, b, t, c["dloss"])
    model = ce_model(h, w, b, t, c["path"], c["dloss"], c["chunk"])
    floor = ce_floor(h, w, b, t, c["dloss"], dt)
    keys = [k for k in ("loss", "dh", "dW", "db") if exact[k] is not None]
    E = {k: float((model[k] - exact[k]).abs().max()) for k in keys}
    allowed = {k: K * E[k] + floor[k] for k in keys}
    n_chunks = -(-N // c["chunk"])
    case = dict(h=h, w=w, b=b, t=t, exact=exact, model=model, E=E,
                allowed=allowed, keys=keys, n_chunks=n_chunks,
                db_sum_allowed=None if b is None else
                db_sum_bound(model, b.dtype, n_chunks, c["dloss"]))
    _e2e_cache[key] = case
    return case
