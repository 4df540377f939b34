"""Perona-Malik in the ORACLE'S operation order (oracle/cv_oracle.c, cvo_perona_malik_channel), restated in numpy and generic over the
dtype: in float64 it is the oracle bit for bit (tests/test_pm_ref.py), in long double it is the high-precision reference the FP64 planes
of the device kernels are held against (tests/test_gpu_pm_state.py).  np_restatement.pm_step associates the Sobel sums differently and is
not bit-equal to the oracle; it stays the independent restatement it was written as.

Order of operations, per step:  Sobel dx = row pass [-1 0 1] (I[j+1] - I[j-1]), then column pass (r[i-1] + r[i]*2) + r[i+1];
dy = row pass (I[j-1] + I[j]*2) + I[j+1], then column pass r[i+1] - r[i-1]; replicated borders;  g = 1 / (1 + (gx*gx + gy*gy) / (K*K)),
1 on the border ring;  s = (((gS + g)(IS - I) + (gE + g)(IE - I)) + (gN + g)(IN - I)) + (gW + g)(IW - I);  I' = I + (L * s) / 4."""
import functools

import numpy as np


def pm_step(I, K, L):
    """One time step on the 2-D plane I in I's own dtype; K and L are taken as the doubles the library and the oracle receive."""
    dt = I.dtype.type
    K, L = dt(float(K)), dt(float(L))
    one, two, four = dt(1), dt(2), dt(4)
    h, w = I.shape
    p = np.pad(I, 1, mode="edge")
    c = p[:, 1:-1]                                   # rows padded, columns as I
    r = np.pad(p[1:-1, 2:] - p[1:-1, :-2], ((1, 1), (0, 0)), mode="edge")
    gx = (r[:-2] + r[1:-1] * two) + r[2:]
    r = (p[:, :-2] + c * two) + p[:, 2:]             # on the padded rows: the pad IS the clamped row
    gy = r[2:] - r[:-2]
    g = one / (one + (gx * gx + gy * gy) / (K * K))
    g[0, :] = one; g[-1, :] = one; g[:, 0] = one; g[:, -1] = one
    gp = np.pad(g, 1, mode="edge")
    s = (gp[2:, 1:-1] + g) * (p[2:, 1:-1] - I)
    s = s + (gp[1:-1, 2:] + g) * (p[1:-1, 2:] - I)
    s = s + (gp[:-2, 1:-1] + g) * (p[:-2, 1:-1] - I)
    s = s + (gp[1:-1, :-2] + g) * (p[1:-1, :-2] - I)
    assert s.dtype == I.dtype and s.shape == (h, w)
    return I + L * s / four


def perona_malik(img, K, L, trips, dtype=np.float64):
    """`trips` steps from the uint8 plane `img`: the state in `dtype`."""
    I = np.asarray(img).astype(dtype)
    for _ in range(trips):
        I = pm_step(I, K, L)
    return I


def to_u8(state):
    """The uint8 plane of a state: cvRound (round half to even), saturated -- what pm_store_kernel and the oracle do."""
    return np.clip(np.rint(state), 0, 255).astype(np.uint8)


def rand_plane(h, w, extra=0):
    """The random uint8 plane of a shape: the seed comes from the shape (and the channel, for planes beyond the first)."""
    return np.random.default_rng(1000 * h + w + 7919 * extra).integers(0, 256, size=(h, w), dtype=np.uint8)


# the (K, L, T) sets the cases draw from: strong / weak edge stopping, L below its cap, 15 to 80 trips
P30, P10, P1000, P100 = (30, 0.25, 5), (10, 0.25, 20), (1000, 0.1, 1.5), (100, 0.25, 10)

# Every (shape, (K, L, T)) the GPU tests run on a random plane: listed once so that tests/test_pm_ref.py validates the restatement and
# computes D_ref on exactly these.  2, 3 and 35 trips (T = 0.5, 0.75, 8.75 with L = 0.25) are the two-step wave kernel's cases.
T2, T3, T35 = (30, 0.25, 0.5), (10, 0.25, 0.75), (100, 0.25, 8.75)
CASES = [
    # tile kernel: one tile, single row / column (all ring), one tile past 32 x 64 in both directions
    ((3, 3), P30), ((1, 50), P10), ((50, 1), P1000), ((33, 65), P100),
    # wave kernel: 60 columns per wave, 240 per workgroup
    ((17, 61), P10), ((9, 241), P30),
    # two-step wave kernel: 56 columns per wave, 224 per workgroup
    ((17, 57), T2), ((17, 57), T3), ((17, 57), T35), ((9, 225), T2), ((9, 225), T3), ((9, 225), T35),
    # resident kernel
    ((16, 16), P30), ((18, 130), P10), ((37, 130), P1000), ((70, 372), P100),
    # batch members with their own K, L, T
    ((16, 16), P100), ((18, 130), P1000), ((40, 56), P10), ((17, 61), P30),
]
CASES = list(dict.fromkeys(CASES))
# CPU only (tests/test_pm_ref.py): shapes of test_perona_malik_parity, for orientation -- D_ref there is 5e-14 .. 1.1e-12
ORIENTATION = [((40, 56), P30), ((64, 64), P10), ((37, 130), P1000), ((70, 372), (30, 0.25, 4)), ((64, 64), (1000, 0.25, 20))]


@functools.lru_cache(maxsize=None)
def reference(shape, klt, extra=0):
    """(img, trips, I_ld) of a case: the long-double state, computed once per session and shared (treat as read-only)."""
    K, L, T = klt
    img = rand_plane(shape[0], shape[1], extra)
    trips = 0
    t = 0.0
    while t < T:           # src/main.cpp:498: the counter is a double
        t += L
        trips += 1
    I_ld = perona_malik(img, K, L, trips, np.longdouble)
    img.setflags(write=False)
    I_ld.setflags(write=False)
    return img, trips, I_ld


# ---- exact ties: planes on which one step with L = T = 0.25 and g == 1 lands on k + 0.5 ----
# With g == 1 everywhere, I1 = I0 + 0.25 * (2 * sum dI) / 4 = I0 + (sum of the four dI) / 8, exact in both arithmetic flavours (small
# integers, powers of two).  Along a line, x = 2 j^2 has second difference +4: I1 = x + 0.5 with x even; x = 250 - 2 j^2 has -4:
# I1 = (x - 1) + 0.5 with x - 1 odd.
TIE_K, TIE_L, TIE_T = 30.0, 0.25, 0.25
_J = np.arange(12)
TIE_LINE = np.concatenate([2 * _J * _J, 250 - 2 * _J * _J]).astype(np.uint8)      # 24 pixels: 10 even ties, 10 odd ties
# g == 1 on every pixel of ANY shape: K so large that (gx^2 + gy^2) / K^2 < 2^-53, so 1 + it rounds to 1 (STRICT) and
# fma(s, 1/K^2, 1) = 1, whose reciprocal is exact (FAST)
TIE_K_FLAT = 1e30


def count_ties(state):
    """(ties with even k, ties with odd k) among the values k + 0.5 of a state."""
    fl = np.floor(state)
    tie = (state - fl) == 0.5
    return int((tie & (fl % 2 == 0)).sum()), int((tie & (fl % 2 == 1)).sum())
