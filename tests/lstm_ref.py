"""fp64 references for the LSTM kernels (plain torch, no project code).

``ref_exact`` is the mathematical LSTM layer in fp64. ``ref_model`` is the
same arithmetic with the roundings each HIP driver performs when it stores
a value (bf16/fp32 stores, e4m3 quantisation), still evaluated in fp64 in
between. The distance between the two is the error a correct kernel is
entitled to; the GPU tests derive their bounds from it.

Layouts: ``x`` is batch-first (B,T,In) like the public op; everything
returned is time-major (T,B,·) like the kernels' saves. Gate order i,f,g,o.
"""
import torch

DRIVERS = ("lib_fp32", "lib_bf16", "fused", "gemv", "gemv_persistent",
           "gemv_fp8", "lib_fp8")


def driver_dtype(driver):
    return torch.float32 if driver == "lib_fp32" else torch.bfloat16


def ref_exact(x, h0, c0, w_ih, w_hh, b_ih, b_hh, gate_perm=(0, 1, 2, 3),
              j_shift=0):
    """fp64 LSTM layer. Returns (hs, cs, gates) time-major, gates
    post-activation; differentiable w.r.t. every argument.

    ``gate_perm`` / ``j_shift`` exist only to build deliberately WRONG
    variants (gate blocks permuted, hidden-unit index rotated) so a test can
    show its bound would catch such an error; the defaults are the LSTM."""
    x, h0, c0, w_hh, b_ih, b_hh = (
        t.double() for t in (x, h0, c0, w_hh, b_ih, b_hh))
    B, T, _ = x.shape
    H = w_hh.shape[1]
    # w_ih=None: x already is the input projection x @ w_ih^T, (B,T,4H)
    xp = (x if w_ih is None else x @ w_ih.double().t()) + (b_ih + b_hh)
    h, c = h0, c0
    hs, cs, gs = [], [], []
    for t in range(T):
        pre = xp[:, t] + h @ w_hh.t()
        blocks = list(pre.split(H, dim=1))
        blocks = [blocks[p] for p in gate_perm]
        if j_shift:
            blocks = [b.roll(j_shift, dims=1) for b in blocks]
        i, f, g, o = blocks
        i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.cat([i, f, g, o], dim=1))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def _rnd(t, dtype):
    """Round an fp64 tensor through a storage type."""
    return t.to(dtype).double()


def _e4m3(t):
    """Saturating e4m3 cast of an fp32-valued tensor, back in fp64."""
    return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double()


def quantize_rows_e4m3(w):
    """Per-row e4m3 weight quantisation of the serving GEMV path:
    returns (q as uint8 (4H,H), fp32 row scales (4H))."""
    scale = w.abs().amax(dim=1, keepdim=True).float().clamp_min(1e-12) / 448.0
    q = (w.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.squeeze(1).contiguous()


def quantize_tensor_e4m3(w):
    """Per-tensor e4m3 quantisation of the training fp8 path:
    returns (q as float8_e4m3fn, fp32 scalar scale)."""
    scale = (w.abs().amax().float() / 448.0).clamp_min(1e-12)
    q = (w.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q, scale


def ref_model(x, h0, c0, w_ih, w_hh, b_ih, b_hh, driver):
    """fp64 arithmetic with ``driver``'s storage roundings. Inputs must
    already hold values representable in the driver's dtype."""
    assert driver in DRIVERS, driver
    dt = driver_dtype(driver)
    F32 = torch.float32
    x, h0, c0, b_ih, b_hh = (t.double() for t in (x, h0, c0, b_ih, b_hh))
    B, T, _ = x.shape
    H = w_hh.shape[1]
    # the projection GEMM's output is stored in dt
    xp = _rnd(x if w_ih is None else x @ w_ih.double().t(), dt)
    bias = _rnd(_rnd(b_ih + b_hh, dt), F32)     # summed in dt, kept fp32
    if driver == "gemv_fp8":
        q, s = quantize_rows_e4m3(w_hh)
        w = q.view(torch.float8_e4m3fn).double() * s.double()[:, None]
    elif driver == "lib_fp8":
        q, s = quantize_tensor_e4m3(w_hh)
        w = q.double() * s.double()
    else:
        w = w_hh.double()
    rec_dt = dt if driver in ("lib_fp32", "lib_bf16", "lib_fp8") else F32
    h_fb = _rnd(h0, dt)                         # what the recurrent GEMM reads
    if driver == "lib_fp8":
        h_fb = _e4m3(h_fb * 448.0) / 448.0
    c = _rnd(c0, F32)
    hs, cs, gs = [], [], []
    for t in range(T):
        rec = _rnd(h_fb @ w.t(), rec_dt)
        pre = _rnd(xp[:, t] + rec + bias, F32)
        i, f, g, o = pre.split(H, dim=1)
        i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
        c = _rnd(f * c + i * g, F32)
        h = _rnd(o * torch.tanh(c), F32)
        hs.append(_rnd(h, dt))
        cs.append(c)
        gs.append(_rnd(torch.cat([i, f, g, o], dim=1), dt))
        # lib_fp8 quantises the UNROUNDED fp32 h with the fixed 1/448 scale
        h_fb = _e4m3(h * 448.0) / 448.0 if driver == "lib_fp8" else hs[-1]
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def cell_backward_exact(dh, dhT, dcT, gates, c_prev, c_t, w_hh):
    """Closed-form fp64 backward of ONE cell (T = 1) from the saved
    post-activation gates: returns (dgates (B,4H), dh0, dc0)."""
    dh, dhT, dcT, gates, c_prev, c_t, w_hh = (
        t.double() for t in (dh, dhT, dcT, gates, c_prev, c_t, w_hh))
    H = w_hh.shape[1]
    i, f, g, o = gates.split(H, dim=1)
    dhe = dh + dhT
    tc = torch.tanh(c_t)
    dct = dcT + dhe * o * (1 - tc * tc)
    dgates = torch.cat([dct * g * i * (1 - i),
                        dct * c_prev * f * (1 - f),
                        dct * i * (1 - g * g),
                        dhe * tc * o * (1 - o)], dim=1)
    return dgates, dgates @ w_hh, dct * f


# ---- forward cases shared by the CPU guard test and the GPU tests --------

# allowed = K * E + floor, E = max|ref_model - ref_exact| (see forward_case).
# K = 2 lets the kernel's roundings fall differently from the model's.
K_FACTOR = {d: 2 for d in DRIVERS}
BF16_HALF_ULP = 2.0 ** -9       # bf16 half-ulp at 1; hs and gates are < 1
FP32_CS_FLOOR = 1e-5
FP32_DRIVER_TOL = 2e-4          # the suite's long-standing fp32 bound

FORWARD_SHAPES = {              # (B, H)
    "lib_fp32": [(3, 8), (5, 6), (2, 3)],
    "lib_bf16": [(3, 24), (5, 20), (2, 5), (67, 8)],
    "fused": [(16, 8), (128, 64), (130, 72), (128, 96)],
    "gemv": [(b, h) for b in (1, 8) for h in (8, 50, 520)],
    "gemv_persistent": [(b, h) for b in (1, 8) for h in (8, 50, 520)],
    "gemv_fp8": [(b, h) for b in (1, 8) for h in (16, 50, 1040)],
    "lib_fp8": [(16, 16), (32, 48)],
}
FORWARD_T = (1, 3)

_WRONG = [dict(gate_perm=p) for p in
          ((1, 0, 2, 3), (2, 1, 0, 3), (3, 1, 2, 0),
           (0, 2, 1, 3), (0, 3, 2, 1), (0, 1, 3, 2))] + [dict(j_shift=1)]


def draw_inputs(driver, B, H, T, seed=0):
    """Random inputs already rounded to the driver's dtype, so kernel and
    reference see the same numbers. Non-zero carried state, |h0| < 1."""
    dt = driver_dtype(driver)
    # 0.3 up to H = 64, then ~1/sqrt(H): the recurrent sum keeps a spread of
    # about 1, so gates stay off saturation (where any error would vanish)
    # and the e4m3 weight error does not swamp the bound at H = 1040
    w_scale = 0.3 * min(1.0, 8.0 / H ** 0.5)
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 13 * H + T)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(
        xp=(0.5 * r(T, B, 4 * H)).to(dt),
        bias=(0.3 * r(4 * H)).to(dt).float(),
        h0=(0.5 * r(B, H)).clamp(-0.98, 0.98).to(dt),
        c0=0.5 * r(B, H),
        w_hh=(w_scale * r(4 * H, H)).to(dt))


_case_cache = {}


def forward_case(driver, B, H, T):
    """Inputs, fp64 exact outputs and the allowed error per output for one
    forward case; computed once and shared (treat as read-only)."""
    key = (driver, B, H, T)
    if key in _case_cache:
        return _case_cache[key]
    inp = draw_inputs(driver, B, H, T)
    zeros = torch.zeros(4 * H)
    args = (inp["xp"].transpose(0, 1), inp["h0"], inp["c0"], None,
            inp["w_hh"], inp["bias"], zeros)
    exact = dict(zip(("hs", "cs", "gates"), ref_exact(*args)))
    model = dict(zip(("hs", "cs", "gates"), ref_model(*args, driver)))
    E = {k: float((model[k] - exact[k]).abs().max()) for k in exact}
    if driver == "lib_fp32":
        allowed = {k: FP32_DRIVER_TOL for k in exact}
    else:
        K = K_FACTOR[driver]
        allowed = {"hs": K * E["hs"] + BF16_HALF_ULP,
                   "gates": K * E["gates"] + BF16_HALF_ULP,
                   "cs": K * E["cs"] + FP32_CS_FLOOR}
    # how far a permutation error would move each output (smallest over
    # the wrong variants): must exceed the bound for the bound to mean much
    moved = {k: float("inf") for k in exact}
    for wrong in _WRONG:
        bad = dict(zip(("hs", "cs", "gates"), ref_exact(*args, **wrong)))
        for k in exact:
            moved[k] = min(moved[k],
                           float((bad[k] - exact[k]).abs().max()))
    case = dict(inp=inp, exact=exact, E=E, allowed=allowed, moved=moved)
    _case_cache[key] = case
    return case


def all_forward_cases():
    return [(d, B, H, T) for d in DRIVERS for (B, H) in FORWARD_SHAPES[d]
            for T in FORWARD_T]
