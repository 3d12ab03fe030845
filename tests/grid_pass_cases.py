"""The shapes at which the capped-grid support kernels make more than one pass of their grid, once, with the inputs and the
plain references the tests of those shapes share (tests/test_grid_passes_host.py checks the claims on the CPU through the
library's own plan queries, tests/test_grid_passes_gpu.py runs the kernels).

A launch of this family caps its grid on the host and its kernel walks the n items with `for (i = ...; i < n; i += one pass)`;
`_native.plan_passes(launch, n)` / `_native.plan_loader(B, n_out)` report the grid from the function the launch site calls."""
import numpy as np

F32 = np.float32

# ------------------------------------------------------------------------------------------ pass plans
EW_N = 1_049_349                          # ww_add_relu_fwd / ww_relu_mask_bwd: odd, 773 floats into the second pass
EW_TINY = (1, 5)
POOL_SHAPE = (4, 260, 260, 64)            # fp32 ww_maxpool3x3s2_fwd / _bwd (B, H, W, C)
DPRE_SHAPE = (4, 4100, 4, 256, 1, 1)      # ww_tconv1d_bwd (B, T, Cin, Cout, k, d): 16 rows of 64 float4s into the second pass
DPRE_SCALE = 2.0
PROJ_SHAPE = (1040, 64, 256)              # ww_gru_fwd, 16-bit modes (B, T, I): the second trip converts the last 1024 rows of x and W_ih
PROJ_SAMPLES = (0, 1023, 1024, 1039)      # first sample, the two around the trip boundary (row 65 536 = sample 1024), last sample
WINDOW_W = 4099                           # ww_wave_windows: windows 4096 .. 4098 are the second trip of workgroups 0 .. 2
WINDOW_CHUNKS = (250, 251)

# ww_dropout_bt (B, T, C), p, seed, step, sample_offset, stream id
DROP_BIG = dict(shape=(2, 4096, 1024), p=0.3, seed=3, step=4, sample_offset=0, stream_id=15)       # t = 4095, c >> 2 = 255, stream 15
DROP_RAGGED = dict(shape=(33, 1000, 127), p=0.3, seed=9, step=1, sample_offset=7, stream_id=2)     # 1 056 000 quads, the last one partial
DROP_SMALL = {
    **{f"c{c}": dict(shape=(3, 7, c), p=0.3, seed=1, step=2, sample_offset=0, stream_id=1) for c in range(1, 6)},
    "seed_step_64bit": dict(shape=(3, 7, 5), p=0.3, seed=2 ** 32 + 12345, step=2 ** 33 + 7, sample_offset=0, stream_id=3),
    "offset_wraps": dict(shape=(6, 5, 9), p=0.3, seed=1, step=2, sample_offset=2 ** 32 - 3, stream_id=4),
    "offset_2_40": dict(shape=(6, 5, 9), p=0.3, seed=1, step=2, sample_offset=2 ** 40 + 5, stream_id=4),
    "p0": dict(shape=(3, 7, 5), p=0.0, seed=1, step=2, sample_offset=0, stream_id=0),
    "p999": dict(shape=(8, 100, 64), p=0.999, seed=5, step=6, sample_offset=0, stream_id=0),
}
DROP_STRIDED = dict(shape=(3, 7, 10), p=0.3, seed=11, step=3, sample_offset=1, stream_id=5, ld_x=17, col_x=3, ld_out=23, col_out=5)


def _quads(shape):
    B, T, C = shape
    return B * T * ((C + 3) // 4)


def pass_cases():
    """name -> (launch of _native.PASS_LAUNCHES, n items as that launch counts them, whole passes only).  Every case is past one
    pass; all but DROP_BIG -- exactly two passes, the shape that puts both counter fields at their limits -- end in a short one."""
    B, H, W, C = POOL_SHAPE
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Bd, Td, _, Cout, _, _ = DPRE_SHAPE
    Bp, Tp, Ip = PROJ_SHAPE
    return {
        "add_relu / relu_mask": ("ew", EW_N, False),
        "maxpool fwd": ("ew", B * Ho * Wo * (C // 4), False),
        "maxpool bwd": ("ew", B * H * W * (C // 4), False),
        "tconv dpre": ("ew", Bd * Td * Cout // 4, False),
        "dropout (33, 1000, 127)": ("dropout_bt", _quads(DROP_RAGGED["shape"]), False),
        "dropout (2, 4096, 1024)": ("dropout_bt", _quads(DROP_BIG["shape"]), True),
        "wave windows": ("wave_windows", WINDOW_W, False),
        "to16_pair": ("to16_pair", (Bp * Tp * Ip + 3 * 128 * Ip) // 4, False),
    }


# the loader: n_out odd (destination rows alternate between 16-byte and 2-byte alignment), 768 whole chunks = 3 passes of 256
LOADER = dict(n_out=6151, L=6188, n_clips=24, rank=2, world=3, k0=64, seed=5, epochs=(0, 3))
LOADER_RUNS = ((1100, True), (2048, True), (2048, False))          # (B, training): S = 2 of 3 passes, then S = 1 of 3
LOADER_TRIPS = {1100: (2, 1), 2048: (3,)}                         # trips of workgroup s of a row


# ------------------------------------------------------------------------------------------ inputs and references
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def same_floats(got, ref):
    """Bit for bit where the reference is a number, NaN exactly where it is NaN."""
    got, ref = np.asarray(got, dtype=F32), np.asarray(ref, dtype=F32)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(ref)[~nan])


SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 1.0, -1.0], dtype=F32)      # 1e-40 is subnormal


def ew_inputs(n, seed=0):
    """(a, b) float32 (n,): N(0,1) with every ordered pair of SPECIALS planted from element 0 on (81 pairs: inside the first
    256), from element 1 048 576 on (the second pass) where n reaches that far, and (as far as they fit) at the very end."""
    rng = np.random.default_rng(seed + n)
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    pa, pb = np.repeat(SPECIALS, len(SPECIALS)), np.tile(SPECIALS, len(SPECIALS))
    for at in (0, 1 << 20, n - len(pa)):
        if at == 0 or at >= (1 << 20):
            m = max(0, min(len(pa), n - at))
            a[at:at + m], b[at:at + m] = pa[:m], pb[:m]
    return a, b


def add_relu_ref(a, b):
    """where(a + b < 0, 0, a + b) in float32: a NaN stays a NaN and -0 stays -0."""
    with np.errstate(invalid="ignore"):
        v = (a + b).astype(F32)
        return np.where(v < 0, F32(0), v)


def relu_mask_ref(dy, y):
    """where(y != 0, dy, 0): zeros of either sign stop the gradient, a NaN in y passes it."""
    return np.where(y != 0, dy, F32(0)).astype(F32)


def window_recording(chunk, order):
    """A recording of WINDOW_W windows whose second-trip windows 4096 .. 4098 are, for order = 'zero_tiny': all zero, peak 1e-30,
    holding a NaN; for 'tiny_zero': peak 1e-30, all zero, holding a NaN (neighbouring windows share half their samples, and
    only the tail of the last window belongs to one window alone, so the NaN is always there).  The first-trip windows of the
    same workgroups differ from them in both directions: window 0 has a peak near 1 (zero_tiny) or near 1e-33 (tiny_zero),
    windows 1 and 2 peaks near 1e-33 -- below 1e-30, above 0."""
    rng = np.random.default_rng(chunk)
    half = chunk // 2
    S = chunk + (WINDOW_W - 1) * half + 7
    wave = (rng.normal(0, 0.2, S) * rng.choice([1e-3, 0.05, 1.0, 30.0], S)).astype(F32)
    quiet = lambda n: (rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n) * 1e-33).astype(F32)
    lo = half if order == "zero_tiny" else 0
    wave[lo:2 * half + chunk] = quiet(2 * half + chunk - lo)
    if order == "zero_tiny":
        wave[:half] = rng.uniform(-1, 1, half).astype(F32)
        wave[3] = F32(0.97)
    s0, s1, s2 = 4096 * half, 4097 * half, 4098 * half
    zero, tiny = (s0, s1) if order == "zero_tiny" else (s1, s0)
    wave[tiny:tiny + chunk] = (rng.uniform(-1, 1, chunk) * 1e-30).astype(F32)
    wave[tiny + (chunk - 1 if tiny == s1 else 0)] = F32(1e-30)     # in the half the zero window does not take
    wave[zero:zero + chunk] = 0.0
    tail = s2 + chunk - half + 1                                   # first sample that only window 4098 holds
    wave[tail:] = (rng.uniform(-1, 1, S - tail) * 0.3).astype(F32)
    wave[S - 12] = np.nan
    return wave


def dropout_case_x(shape, seed=0):
    """float32 (B, T, C): N(0,1) with -0 and NaN planted on a regular pattern (kept and dropped ones of each occur)."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    flat = x.reshape(-1)
    flat[0::7] = F32(-0.0)
    flat[3::11] = np.nan
    return x


def dropout_p32(p):
    return float(F32(p))


def dropout_ref(x, keep, p):
    """where(keep, float32(x) * float32(scale), +0), scale = float32(1 / (1 - float(float32(p)))): one IEEE multiply."""
    scale = F32(1.0 / (1.0 - dropout_p32(p)))
    with np.errstate(invalid="ignore"):
        return np.where(keep, np.asarray(x, dtype=F32) * scale, F32(0)).astype(F32)


def dropout_keep(case):
    from oracle.gru import dropout_bt_mask
    B, T, C = case["shape"]
    return dropout_bt_mask(B, T, C, dropout_p32(case["p"]), case["seed"], case["step"], case["sample_offset"], case["stream_id"])


_KEEP = {}


def dropout_keep_cached(name, case):
    """The big masks are drawn once per process (a second of NumPy Philox each)."""
    if name not in _KEEP:
        _KEEP[name] = dropout_keep(case)
    return _KEEP[name]
