"""Helper of the optimiser tests (no test in here): the fp64 yardstick of global-norm clipping + AdamW, the per-element bounds the engine's
step is held to, a numpy-float32 emulation of the kernel's formula (posediffusion_amd/csrc/pd_optim.hip, pd_opt_adamw_elem), and the
input sets that tests/test_optim_cpu.py runs the emulation on and tests/test_gpu_optim.py runs the engine on.

Bounds, with u_abs = (lr / (1 - b1^step)) (b1 |m0| + (1 - b1) |g coef64|) / (sqrt(v64) / sqrt(1 - b2^step) + eps):
    norm  |norm - norm64| <= 2^-22 norm64                               fp64 accumulation, one rounding and the sqrt; 4x margin
    m     |m - m64| <= 8 2^-24 (b1 |m0| + (1 - b1) |g coef64|)          three roundings plus the coefficient's ~ 4 units
    v     |v - v64| <= 16 2^-24 v64 + 2^-120                            the coefficient enters squared; g^2 may underflow in fp32
    p     |p - p64| <= 2 ulp(max(|p64|, |p0|)) + 32 2^-24 u_abs         two roundings on p, ~ 20 in m / denom
u_abs and not |u|: m can cancel to near zero while its absolute error does not."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24

CHUNK = 4096   # posediffusion_amd.optim.CHUNK (tests/test_optim_cpu.py checks the two against each other and against the header)


def sizes(chunk=CHUNK):
    """The size list of the tests: one element, around a wavefront, around a workgroup, around one chunk, several chunks and a tail."""
    return [1, 3, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]


HP = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def hp(**kw):
    return dict(HP, **kw)


# ---- the fp64 yardstick -------------------------------------------------------------------------
def norm64(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, F64) ** 2)) for g in grads)))


def coef64(norm, max_norm):
    """clamp(max_norm / (norm + 1e-6), max = 1); 1 without clipping"""
    if max_norm is None:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def step64(p0, g, m0, v0, step, h, coef):
    """One AdamW step in fp64 from fp32 inputs: (p, m, v, u_abs, m_abs)."""
    p0, g, m0, v0 = (np.asarray(a, F64) for a in (p0, g, m0, v0))
    b1, b2 = h["betas"]
    gc = g * coef
    m = b1 * m0 + (1.0 - b1) * gc
    v = b2 * v0 + (1.0 - b2) * gc * gc
    step_size = h["lr"] / (1.0 - b1 ** step)
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + h["eps"]
    p = p0 * (1.0 - h["lr"] * h["weight_decay"]) - step_size * m / denom
    m_abs = b1 * np.abs(m0) + (1.0 - b1) * np.abs(gc)
    return p, m, v, step_size * m_abs / denom, m_abs


def ulp32(x):
    """the fp32 unit in the last place at |x| (x in fp64)"""
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def bounds(p0, g, m0, v0, step, h, coef):
    """(p64, m64, v64, p_bound, m_bound, v_bound)"""
    p, m, v, u_abs, m_abs = step64(p0, g, m0, v0, step, h, coef)
    pb = 2.0 * ulp32(np.maximum(np.abs(p), np.abs(np.asarray(p0, F64)))) + 32.0 * U * u_abs
    return p, m, v, pb, 8.0 * U * m_abs, 16.0 * U * v + 2.0 ** -120


def norm_bound(n64):
    return 2.0 ** -22 * n64


def worst(x, x64, bound):
    """max of |x - x64| / bound (0 / 0 counts as 0, anything / 0 as inf)"""
    err = np.abs(np.asarray(x, F64) - x64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def check_case(case, p_new, m_new, v_new, norm=None):
    """The engine's (or the emulation's) results of `case` against the yardstick: {quantity: worst error / bound}, every one <= 1 to pass."""
    n64 = norm64(case["g"])
    coef = coef64(n64, case["max_norm"])
    out = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i in range(len(case["p"])):
        h = case["groups"][case["group"][i]]
        p, m, v, pb, mb, vb = bounds(case["p"][i], case["g"][i], case["m"][i], case["v"][i], case["step"][i], h, coef)
        out["p"] = max(out["p"], worst(p_new[i], p, pb))
        out["m"] = max(out["m"], worst(m_new[i], m, mb))
        out["v"] = max(out["v"], worst(v_new[i], v, vb))
    if norm is not None:
        out["norm"] = abs(float(norm) - n64) / norm_bound(n64) if n64 > 0 else float(float(norm) != 0.0)
    return out


# ---- the kernel's formula in numpy float32 ------------------------------------------------------
def _fma32(a, b, c):
    # a b is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding: off by one fp32 unit in rare ties)
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def norm32(grads):
    """the engine's norm: squares and sum in fp64, square root in fp64, one rounding to fp32"""
    return F32(np.sqrt(sum(float(np.sum(np.asarray(g, F64) ** 2)) for g in grads)))


def coef32(norm, max_norm):
    c = F32(max_norm) / (F32(norm) + F32(1e-6))
    return F32(1.0) if c > F32(1.0) else c          # a NaN stays a NaN


def step32(p0, g, m0, v0, step, h, coef=None):
    """pd_opt_adamw_elem operation by operation: the scalars are formed in double and rounded to fp32, every operation rounds to fp32."""
    b1, b2 = h["betas"]
    decay, fb1, omb1, fb2, omb2 = F32(1.0 - h["lr"] * h["weight_decay"]), F32(b1), F32(1.0 - b1), F32(b2), F32(1.0 - b2)
    step_size, bc2_sqrt, eps = F32(h["lr"] / (1.0 - b1 ** step)), F32(np.sqrt(1.0 - b2 ** step)), F32(h["eps"])
    p0, g, m0, v0 = (np.asarray(a, F32) for a in (p0, g, m0, v0))
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        if coef is not None:
            g = g * F32(coef)
        pd = p0 * decay
        m = _fma32(np.broadcast_to(fb1, m0.shape), m0, omb1 * g)
        v = _fma32(np.broadcast_to(fb2, v0.shape), v0, omb2 * (g * g))
        den = np.sqrt(v) / bc2_sqrt + eps
        q = m / den
        p = _fma32(np.broadcast_to(-step_size, q.shape), q, pd)
    return p, m, v


def emulate_case(case):
    """(p, m, v, norm) of `case` by the fp32 emulation"""
    n = norm32(case["g"])
    coef = None if case["max_norm"] is None else coef32(n, case["max_norm"])
    ps, ms, vs = [], [], []
    for i in range(len(case["p"])):
        p, m, v = step32(case["p"][i], case["g"][i], case["m"][i], case["v"][i], case["step"][i], case["groups"][case["group"][i]], coef)
        ps.append(p), ms.append(m), vs.append(v)
    return ps, ms, vs, n


# ---- input sets ---------------------------------------------------------------------------------
def make_case(name, groups=None, group=None, steps=1, gscale=1.0, grad="randn", p_zero=False, max_norm=None, seed=0, size_list=None):
    """One step's inputs as lists of fp32 arrays.  steps: the count AFTER this step, one for all or one per tensor (cycled); a tensor at
    step 1 starts from no state (m = v = 0), a later one from a loaded state at the gradient's scale."""
    rng = np.random.default_rng(seed)
    size_list = sizes() if size_list is None else size_list
    groups = [hp()] if groups is None else groups
    n = len(size_list)
    steps = [steps] * n if isinstance(steps, int) else [steps[i % len(steps)] for i in range(n)]
    case = dict(name=name, groups=groups, group=[0] * n if group is None else [group[i % len(group)] for i in range(n)], step=steps,
                max_norm=max_norm, p=[], g=[], m=[], v=[])
    for i, sz in enumerate(size_list):
        case["p"].append(np.zeros(sz, F32) if p_zero else rng.standard_normal(sz).astype(F32))
        if grad == "zero":
            g = np.zeros(sz, F32)
        elif grad == "tiny":
            g = np.full(sz, 1e-30, F32) * np.where(rng.random(sz) < 0.5, F32(-1), F32(1))
        else:
            g = (rng.standard_normal(sz) * gscale).astype(F32)
        case["g"].append(g)
        if steps[i] == 1:
            case["m"].append(np.zeros(sz, F32)), case["v"].append(np.zeros(sz, F32))
        else:
            case["m"].append((0.3 * gscale * rng.standard_normal(sz)).astype(F32))
            case["v"].append((gscale * gscale * (0.05 + rng.random(sz))).astype(F32))
    return case


def step_cases():
    """test 2 of tests/test_gpu_optim.py: one step against fp64 (no clipping)"""
    return [
        make_case("base", seed=1),
        make_case("step1000", steps=1000, seed=2),
        make_case("wd0", groups=[hp(weight_decay=0.0)], seed=3),
        make_case("wd0_step1000", groups=[hp(weight_decay=0.0)], steps=1000, seed=4),
        make_case("betas_05_09", groups=[hp(betas=(0.5, 0.9))], seed=5),
        make_case("betas_05_09_step1000", groups=[hp(betas=(0.5, 0.9))], steps=1000, seed=6),
        make_case("lr1", groups=[hp(lr=1.0)], seed=7),
        make_case("lr1_step1000", groups=[hp(lr=1.0)], steps=1000, seed=8),
        make_case("two_groups", groups=[hp(), hp(lr=1.0, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.0)], group=[0, 1], steps=[1, 1, 7], seed=9),
        make_case("steps_differ", steps=[1, 2, 5, 1000, 3], seed=10),
        make_case("zero_grad", grad="zero", seed=11),
        make_case("zero_grad_step1000", grad="zero", steps=1000, seed=12),
        make_case("tiny_grad", grad="tiny", seed=13),
        make_case("tiny_grad_step5", grad="tiny", steps=5, gscale=1e-30, seed=14),
        make_case("p_zero", p_zero=True, seed=15),
        make_case("p_zero_lr1_step1000", p_zero=True, groups=[hp(lr=1.0)], steps=1000, seed=16),
    ]


def clip_cases():
    """test 3: the norm above max_norm at three gradient scales (the smallest of them stays below it: the coefficient is exactly 1)"""
    return [make_case(f"clip_g{gs:g}_s{st}", gscale=gs, steps=st, max_norm=1.0, seed=20 + i)
            for i, (gs, st) in enumerate([(1e-3, 1), (1.0, 1), (1e3, 1), (1.0, 1000), (1e3, [1, 4, 1000])])]


def all_cases():
    return step_cases() + clip_cases()


def norm_values(size_list, seed=0):
    """gradients whose magnitudes spread over 1e-20 .. 1e18"""
    rng = np.random.default_rng(seed)
    return [(np.where(rng.random(s) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-20.0, 18.0, s)).astype(F32) for s in size_list]
