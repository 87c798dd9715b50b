"""Named cases, the oracle and the tolerances for the fused Adam step (csrc/gsr_adam.h, csrc/gsr_adam.hip.h:
gsr_adam_step_multi), shared by tests/test_adam_host_cpu.py (the scalar source built for the host, and the tensor-op branch
of gsplat_attack.optim.GaussianAdam), tests/test_optim_cpu.py and tests/test_gpu_adam.py (the kernel, bit for bit the host
build).

Oracle: torch.optim.Adam itself on the CPU (what the reference calls), with the state (step, exp_avg, exp_avg_sq) injected,
one step.  Inputs are exact float32 promoted to float64; lr, the betas and eps take their float32 values.

Tolerance of one step against the float64 oracle, derived, with u = 2^-24 (each float32 operation of csrc/gsr_adam.h rounds
once, relative error <= u; products that underflow add 2^-149 each).  First-order terms, doubled:
  m' = m + w1 (g - m), w1 = 1 - b1: the subtraction, w1 and the product each perturb w1 |g - m| by u, the sum rounds m':
        e_m = 2 u (3 w1 |g - m| + |m'|) + 2 * 2^-149
  v' = b2 v + w2 (g g), w2 = 1 - b2: w2, two products: 3 u w2 g^2; the product b2 v: u b2 v; the sum: u v':
        e_v = 2 u (3 w2 g^2 + b2 v + v') + 4 * 2^-149
  den = sqrt(v') / sqrt_bc2 + eps: the root carries v's error -- sqrt(v' + e_v) - sqrt(max(v' - e_v, 0)), which holds at
  v' = 0 too -- and the root, the rounding of sqrt_bc2 and the division add 3 u sqrt(v') / sqrt_bc2; the sum rounds den:
        e_den = e_root / sqrt_bc2 + 2 (3 u sqrt(v') / sqrt_bc2 + u den)
  q = m' / den:   e_q = e_m / den + |m'| e_den / den^2 + 2 u |q|
  x' = x - step_size q: the rounding of step_size and the product: 2 u step_size |q|; the difference rounds x':
        e_x = step_size e_q + 2 (2 u step_size |q| + u |x'|)

Trajectories (TRAJ_*): 100 steps of a pre-drawn gradient sequence; the measured worst error of the host build is written
down below and 4x it is asserted (the run is deterministic; the margin is for another libm).
For optimiser-level runs of N steps against torch.optim.Adam in float32 (tests/test_optim_cpu.py): trajectory_bound.
"""
import ctypes
import functools
import os

import numpy as np
import torch

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
HM = os.path.join(ROOT, "tests", "host_math")
SRC = os.path.join(HM, "adam_host.cpp")

U = 2.0 ** -24
DENORM = 2.0 ** -149
MAX_TENSORS, MAX_COLS = 8, 48                       # ADAM_* of csrc/gsr_adam.h
F32 = lambda v: float(np.float32(v))                # noqa: E731
FLT_MAX = float(np.finfo(np.float32).max)

SWEEP_COLS = (1, 3, 4, 16, 45, 48)
SWEEP_ROWS = (1, 2, 63, 64, 65, 255, 257, 1025)
SWEEP_T = (1, 2, 10, 1000, 100000)
MODEL_COLS = (3, 3, 45, 1, 3, 4, 16)                # xyz, f_dc, f_rest, opacity, scaling, rotation, obj_dc
MODEL_LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001, 0.0025)

# Measured on the host build (g++ -O1 -ffp-contract=off, glibc): the worst |x_k - reference_k| over the 100 steps and all
# elements of the trajectory case, relative to the largest |x_100 - x_0| of the reference.  Asserted at 4x.
# (against float64 the float32 roundings of x -- half an ulp of |x| up to 4 per step -- add up like a random walk; torch's
# float32 run makes nearly the same roundings, so the two float32 runs stay ten times closer)
TRAJ_ERR_VS_F64 = 2.28e-6
TRAJ_ERR_VS_F32 = 2.41e-7


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = host_build.host_lib("adam")
    lib.ah_step_multi.restype = ctypes.c_int
    lib.ah_step_multi.argtypes = [ctypes.c_int32] + [ctypes.c_void_p] * 10 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    lib.ah_bias.restype = None
    lib.ah_bias.argtypes = [ctypes.c_double] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.ah_expon_lr.restype = ctypes.c_double
    lib.ah_expon_lr.argtypes = [ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_double, ctypes.c_int64]
    lib.ah_span.restype = ctypes.c_int32
    lib.ah_blocks.restype = ctypes.c_uint64
    lib.ah_blocks.argtypes = [ctypes.c_uint64]
    lib.ah_tensor_of_block.restype = ctypes.c_int32
    lib.ah_tensor_of_block.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32]
    lib.ah_row_of.restype = ctypes.c_uint64
    lib.ah_row_of.argtypes = [ctypes.c_uint64, ctypes.c_int32]
    return lib


def span() -> int:
    """ADAM_SPAN: the floats of one tensor a workgroup owns, from the header"""
    return int(host_lib().ah_span())


# ---- the cases ---------------------------------------------------------------------------------------------------------------
class Call:
    """One call of gsr_adam_step_multi: tensors = [(x, g, m, v), ...] read-only float32 [rows, cols]; lr, b1, b2, eps per
    tensor (float32 values); step; mask = None or uint8 [rows]; rows = None or (begin, end); shift[t] = floats past a
    16-byte boundary at which the device test places tensor t."""

    def __init__(self, name, tensors, lr, step, b1=0.9, b2=0.999, eps=1e-15, mask=None, rows=None, shift=None):
        n = len(tensors)
        per = lambda v: [F32(e) for e in (v if isinstance(v, (list, tuple)) else [v] * n)]   # noqa: E731
        self.name, self.step, self.n = name, int(step), n
        self.lr, self.b1, self.b2, self.eps = per(lr), per(b1), per(b2), per(eps)
        self.tensors = []
        for four in tensors:
            arrs = []
            for a in four:
                a = np.ascontiguousarray(a, dtype=np.float32)
                assert a.ndim == 2 and 1 <= a.shape[1] <= MAX_COLS and a.shape == four[0].shape
                a.setflags(write=False)
                arrs.append(a)
            self.tensors.append(tuple(arrs))
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self.rows = None if rows is None else (int(rows[0]), int(rows[1]))
        self.shift = list(shift) if shift is not None else [0] * n
        assert len(self.lr) == len(self.b1) == len(self.b2) == len(self.eps) == len(self.shift) == n

    def live(self, t):
        """bool [rows of tensor t]: the rows that move"""
        R = self.tensors[t][0].shape[0]
        lv = np.ones(R, bool) if self.mask is None else self.mask != 0
        if self.rows is not None:
            inside = np.zeros(R, bool)
            inside[self.rows[0]:self.rows[1]] = True
            lv = lv & inside
        return lv

    def without_selection(self):
        return Call(self.name + "-all", self.tensors, self.lr, self.step, self.b1, self.b2, self.eps, shift=self.shift)


def _rng(name):
    return np.random.default_rng(sum(map(ord, name)) * 7919 + len(name))     # str hashes change per process


def _four(r, rows, cols, zero_state=False):
    """x ~ N(0, 1); g ~ N(0, 1); m ~ N(0, 0.3); v = 0.5 N(0, 1)^2 + 1e-3: every element takes a step of about lr"""
    x = r.standard_normal((rows, cols))
    g = r.standard_normal((rows, cols))
    m = np.zeros((rows, cols)) if zero_state else 0.3 * r.standard_normal((rows, cols))
    v = np.zeros((rows, cols)) if zero_state else 0.5 * r.standard_normal((rows, cols)) ** 2 + 1e-3
    return tuple(a.astype(np.float32) for a in (x, g, m, v))


def sweep_name(cols, rows, t):
    return f"sweep-c{cols}-r{rows}-t{t}"


SWEEP = [sweep_name(c, r, t) for c in SWEEP_COLS for r in SWEEP_ROWS for t in SWEEP_T]
NONFINITE_AT = (2, 1)
NONFINITE_VALUES = {"nan": ("g", float("nan")), "+inf": ("g", float("inf")), "-inf": ("g", float("-inf")), "g+1e-25": ("g", 1e-25),
                    "g-1e-25": ("g", -1e-25), "g+1e19": ("g", 1e19), "g-1e19": ("g", -1e19), "v-fltmax": ("v", FLT_MAX)}
NONFINITE = ["nonfinite-" + k for k in NONFINITE_VALUES]
P_MASK = 1025


def _model_pack(name, P, zero_state=False):
    r = _rng(name)
    return [_four(r, P, c, zero_state) for c in MODEL_COLS]


def boundary_rows(P=P_MASK):
    """the rows on either side of every workgroup span boundary of every tensor of the model pack"""
    S, rows = span(), set()
    for c in MODEL_COLS:
        for e in range(S, P * c, S):
            rows |= {(e - 1) // c, e // c}
    return sorted(rows)


def _masks(P=P_MASK):
    alt = (np.arange(P) % 2).astype(np.uint8)
    only = lambda *rs: np.isin(np.arange(P), rs).astype(np.uint8)   # noqa: E731
    return {"zeros": np.zeros(P, np.uint8), "ones": np.full(P, 1, np.uint8), "alternating": alt, "row0": only(0), "last": only(P - 1),
            "middle": only(P // 2), "boundaries": only(*boundary_rows(P))}


MASKS = ["mask-" + k for k in ("zeros", "ones", "alternating", "row0", "last", "middle", "boundaries")]
RANGES = {"range-0-0": (0, 0), "range-0-1": (0, 1), "range-1024-1025": (1024, 1025), "range-512-513": (512, 513), "range-full": (0, P_MASK)}
MASK_AND_RANGE = "mask-alternating-range-300-700"
SELECT = MASKS + list(RANGES) + [MASK_AND_RANGE]
# designed live-row counts
SELECT_LIVE = {"mask-zeros": 0, "mask-ones": P_MASK, "mask-alternating": P_MASK // 2, "mask-row0": 1, "mask-last": 1, "mask-middle": 1,
               "range-0-0": 0, "range-0-1": 1, "range-1024-1025": 1, "range-512-513": 1, "range-full": P_MASK, MASK_AND_RANGE: 200}
PACKS = ["pack1", "pack7", "pack8", "pack-zero-rows", "pack-misaligned"]
OTHER = ["first-step", "lr0", "nonfinite-base"]
NAMES = SWEEP + PACKS + OTHER + NONFINITE + SELECT


@functools.lru_cache(maxsize=None)
def case(name) -> Call:
    r = _rng(name)
    if name.startswith("sweep-"):
        c, rows, t = (int(p[1:]) for p in name.split("-")[1:])
        return Call(name, [_four(r, rows, c)], 1e-2, t)
    if name == "pack1":
        return Call(name, [_four(r, 257, 3)], 1e-2, 3)
    if name == "pack7":
        return Call(name, _model_pack(name, 257), list(MODEL_LRS), 7)
    if name == "pack8":                            # eight row counts, per-tensor lr / betas / eps
        shapes = [(1, 48), (63, 1), (64, 16), (65, 45), (255, 4), (257, 3), (1025, 2), (2, 5)]
        return Call(name, [_four(r, *s) for s in shapes], [1e-3 * (k + 1) for k in range(8)], 12, b1=[0.9, 0.8, 0.5, 0.0, 0.9, 0.95, 0.99, 0.9],
                    b2=[0.999, 0.99, 0.9, 0.0, 0.999, 0.999, 0.9999, 0.5], eps=[1e-15, 1e-8, 1e-6, 1e-3, 1e-15, 1e-15, 1e-10, 1e-8])
    if name == "pack-zero-rows":
        return Call(name, [_four(r, 0, 3), _four(r, 65, 45), _four(r, 0, 16), _four(r, 257, 4), _four(r, 0, 1)], 1e-2, 2)
    if name == "pack-misaligned":                  # [1:] views: one float off a 16-byte boundary, beside aligned tensors
        return Call(name, [_four(r, 257, 3), _four(r, 257, 45), _four(r, 65, 4), _four(r, 1025, 1), _four(r, 64, 16)], 1e-2, 5,
                    shift=[1, 0, 1, 0, 3])
    if name == "first-step":                       # zero state, t = 1: |dx| = lr wherever |g| >= 1e-10; g = 0 moves nothing
        x, g, m, v = _four(r, 257, 3, zero_state=True)
        g = g.copy()
        g[::5] = 0.0
        g[1::5] *= np.float32(1e-9)
        return Call(name, [(x, g, m, v)], 1e-2, 1)
    if name == "lr0":
        return Call(name, [_four(r, 65, 45), _four(r, 257, 3)], 0.0, 4)
    if name.startswith("nonfinite-"):
        x, g, m, v = (a.copy() for a in _four(_rng("nonfinite-base"), 5, 4))
        if name != "nonfinite-base":
            who, val = NONFINITE_VALUES[name[len("nonfinite-"):]]
            (g if who == "g" else v)[NONFINITE_AT] = val
        return Call(name, [(x, g, m, v)], 1e-2, 3)
    if name in SELECT:
        pack = _model_pack("select", P_MASK)       # the same inputs under every selection
        mask = rows = None
        if name == MASK_AND_RANGE:
            mask, rows = _masks()["alternating"], (300, 700)
        elif name in RANGES:
            rows = RANGES[name]
        else:
            mask = _masks()[name[len("mask-"):]]
        return Call(name, pack, list(MODEL_LRS), 9, mask=mask, rows=rows)
    raise KeyError(name)


def beyond_root_case() -> Call:
    """nonfinite-base with g = 5e19 at NONFINITE_AT: beyond sqrt(FLT_MAX), where g g overflows (not in NAMES: here the contract
    of csrc/gsr_adam.h differs from torch, which is what tests/test_adam_host_cpu.py states)"""
    x, g, m, v = (a.copy() for a in case("nonfinite-base").tensors[0])
    g[NONFINITE_AT] = 5e19
    return Call("beyond-root-5e19", [(x, g, m, v)], 1e-2, 3)


# ---- the host build ------------------------------------------------------------------------------------------------------------
def host_run(c: Call, lib=None):
    """-> [(x, m, v), ...] after the step through tests/host_math/adam_host.cpp"""
    lib = lib or host_lib()
    bufs = [[a.copy() for a in four] for four in c.tensors]
    n = c.n
    arr = lambda k: (ctypes.c_void_p * n)(*[b[k].ctypes.data if b[k].size else None for b in bufs])   # noqa: E731
    f32 = lambda v: (ctypes.c_float * n)(*v)   # noqa: E731
    rc = lib.ah_step_multi(n, arr(0), arr(1), arr(2), arr(3), (ctypes.c_int64 * n)(*[b[0].shape[0] for b in bufs]),
                           (ctypes.c_int32 * n)(*[b[0].shape[1] for b in bufs]), f32(c.lr), f32(c.b1), f32(c.b2), f32(c.eps), c.step,
                           None if c.mask is None else c.mask.ctypes.data, *((0, -1) if c.rows is None else c.rows))
    assert rc == 0, (c.name, rc)
    for b, four in zip(bufs, c.tensors):
        assert np.array_equal(b[1].view(np.uint32), four[1].view(np.uint32)), "the gradient was written"
    return [(b[0], b[2], b[3]) for b in bufs]


# ---- the oracle: torch.optim.Adam ----------------------------------------------------------------------------------------------
def torch_adam_step(x, g, m, v, lr, b1, b2, eps, step, dtype):
    """torch.optim.Adam on the CPU in `dtype`, state injected (step - 1 steps taken), one step -> (x, m, v) numpy"""
    p = torch.nn.Parameter(torch.from_numpy(np.array(x)).to(dtype))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(np.array(m)).to(dtype),
                        exp_avg_sq=torch.from_numpy(np.array(v)).to(dtype))
    p.grad = torch.from_numpy(np.array(g)).to(dtype)
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == step
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def oracle(c: Call, dtype=torch.float64):
    """-> [(x, m, v), ...]: torch.optim.Adam on the live rows, the inputs on the others"""
    out = []
    for t, (x, g, m, v) in enumerate(c.tensors):
        np_dt = np.float64 if dtype == torch.float64 else np.float32
        res = [x.astype(np_dt), m.astype(np_dt), v.astype(np_dt)]
        lv = c.live(t)
        if lv.any():
            ox, om, ov = torch_adam_step(x[lv], g[lv], m[lv], v[lv], c.lr[t], c.b1[t], c.b2[t], c.eps[t], c.step, dtype)
            res[0][lv], res[1][lv], res[2][lv] = ox, om, ov
        out.append(tuple(res))
    return out


def bounds(c: Call, t: int, ref):
    """(e_x, e_m, e_v) of tensor t from the float64 oracle's results: the derivation at the top"""
    x, g, m, v = (a.astype(np.float64) for a in c.tensors[t])
    ox, om, ov = ref
    b1, b2, eps = c.b1[t], c.b2[t], c.eps[t]
    w1, w2 = 1.0 - b1, 1.0 - b2
    ss = c.lr[t] / (1.0 - b1 ** c.step)
    sb = np.sqrt(1.0 - b2 ** c.step)
    with np.errstate(all="ignore"):
        e_m = 2 * U * (3 * w1 * np.abs(g - m) + np.abs(om)) + 2 * DENORM
        e_v = 2 * U * (3 * w2 * g * g + b2 * v + ov) + 4 * DENORM
        root = np.sqrt(ov)
        e_root = np.sqrt(ov + e_v) - np.sqrt(np.maximum(ov - e_v, 0.0))
        den = root / sb + eps
        e_den = e_root / sb + 2 * (3 * U * root / sb + U * den)
        q = om / den
        e_q = e_m / den + np.abs(om) * e_den / den ** 2 + 2 * U * np.abs(q)
        e_x = ss * e_q + 2 * (2 * U * ss * np.abs(q) + U * np.abs(ox))
    return e_x, e_m, e_v


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def check(label, c: Call, got, ref=None, quiet=True) -> float:
    """got = [(x, m, v), ...] float32: live rows within the derived bounds of the float64 oracle, the others bit for bit their
    inputs -> the worst error / bound"""
    ref = ref or oracle(c)
    worst = 0.0
    for t in range(c.n):
        lv = c.live(t)
        ins = (c.tensors[t][0], c.tensors[t][2], c.tensors[t][3])
        for what, a, b in zip("xmv", got[t], ins):
            assert a.dtype == np.float32 and a.shape == b.shape
            assert np.array_equal(_bits(a[~lv]), _bits(b[~lv])), f"{label} {c.name} tensor {t}: a row left out changed in {what}"
        if not lv.any():
            continue
        for what, a, r, e in zip("xmv", got[t], ref[t], bounds(c, t, ref[t])):
            err = np.abs(a[lv].astype(np.float64) - r[lv])
            ratio = float(np.max(err / e[lv]))
            assert ratio <= 1.0, f"{label} {c.name} tensor {t} {what}: error / bound {ratio:.3f}"
            worst = max(worst, ratio)
    if not quiet:
        print(f"adam {label} {c.name}: worst error / bound {worst:.3f}")
    return worst


def moved_fraction(c: Call, got) -> float:
    n = k = 0
    for t in range(c.n):
        n, k = n + got[t][0].size, k + int((got[t][0] != c.tensors[t][0]).sum())
    return k / max(n, 1)


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def fnv1a(arrays) -> int:
    h = 2166136261
    for a in arrays:
        for byte in np.ascontiguousarray(a, np.float32).tobytes():
            h = ((h ^ byte) * 16777619) & 0xFFFFFFFF
    return h


# ---- trajectories ----------------------------------------------------------------------------------------------------------------
TRAJ_STEPS, TRAJ_LR = 100, 1e-2


@functools.lru_cache(maxsize=None)
def trajectory_inputs():
    """x0 [257, 3] and 100 pre-drawn gradients that do not depend on x (a drifting mean, so that x travels)"""
    r = _rng("trajectory")
    x0 = r.standard_normal((257, 3)).astype(np.float32)
    drift = r.standard_normal((257, 3))
    grads = (drift[None] + r.standard_normal((TRAJ_STEPS, 257, 3))).astype(np.float32)
    x0.setflags(write=False)
    grads.setflags(write=False)
    return x0, grads


@functools.lru_cache(maxsize=None)
def trajectory_reference(dtype):
    """torch.optim.Adam on the CPU over the sequence -> x after every step [100, 257, 3] (numpy, in dtype)"""
    x0, grads = trajectory_inputs()
    p = torch.nn.Parameter(torch.from_numpy(x0.copy()).to(dtype))
    opt = torch.optim.Adam([p], lr=F32(TRAJ_LR), betas=(F32(0.9), F32(0.999)), eps=F32(1e-15))
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g.copy()).to(dtype)
        opt.step()
        out.append(p.detach().clone().numpy())
    res = np.stack(out)
    res.setflags(write=False)
    return res


def trajectory_error(xs, dtype) -> float:
    """xs [100, 257, 3]: the worst |x_k - reference_k| relative to the largest |x_100 - x_0| of the reference"""
    ref = trajectory_reference(dtype).astype(np.float64)
    x0, _ = trajectory_inputs()
    travelled = np.abs(ref[-1] - x0.astype(np.float64)).max()
    assert travelled > 0.5                                 # 100 steps of about lr each in a steady direction
    return float(np.abs(np.asarray(xs, np.float64) - ref).max() / travelled)


def trajectory_bound(steps: int, xmax: float, lr: float) -> float:
    """|x_N - x_N of torch.optim.Adam in float32| per element after N steps of one sequence of gradients, derived: each step
    rounds x once on either side (2 u xmax); the moments pick up at most 4 roundings a step each, so after N steps m / den
    differs by at most 8 N u relative on either side, times a step of at most 4 lr (|m^ / sqrt(v^)| <= (1 - b1) / sqrt(1 -
    b2) < 4 for the reference's betas): 64 N u lr.  Doubled (first order)."""
    return 2.0 * steps * U * (2.0 * xmax + 64.0 * steps * lr)
