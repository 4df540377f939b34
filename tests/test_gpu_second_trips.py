"""The member-table kernels where their lanes, waves and workgroups make a SECOND trip ("Trips"): ingest, image out, mask,
histogram / Otsu, the threshold / rect / disk starts, restrict, prolong, both stages of the energy, the row stages of score and reinit.
Every older test of these operations stays below the cap on a member's workgroups, where the `+= stride` / `+= nblk` branches never run;
here every case passes its cap (test_trip_counts.py pins that on the CPU, from the library's own block functions) with the kernel's
ragged tail alive, and is held to the operation's existing restatement by the operation's existing bar: == or bit patterns for everything
made of integers or copies, test_gpu_energy.check_terms (1e-9 relative to the exactly rounded sums) for the energy.  Each operation with
a batch form also runs as member 1 of 3 -- the one place where a stride taken from the grid, not from the member's section, or a lost
`first` offset shows -- and must give the bits of its single call; score and mask also run in their host forms.
NOT covered: the mid-loop flush of the byte sums (256 trips of a lane): it takes a plane of 2^31 pixels.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import energy_util as E
import init_util as I
import pyramid_util as P
import reinit_util as R
import score_util as S
import trips_util as T
from test_gpu_device_io import Hip, INTERLEAVED, PLANAR, planes_of, rand_image, source_bytes
from test_gpu_energy import check_terms, params_of, restated, same_bits
from test_gpu_reinit import give_levelset

pytestmark = pytest.mark.gpu
NAN = float("nan")
bits = P.bits


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


@pytest.fixture()
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


def closing(ctxs):
    for c in ctxs:
        c.close()


# ---- ingest, image out, mask: 16-pixel pieces, 524 672 of them for 524 288 lanes, and one last pixel ----
@pytest.mark.parametrize("channels", [1, 3])
def test_ingest_mask_and_image_out(capi, hip, channels):
    """Both source layouts at an odd byte offset: the planes are the source's, the plane sums those of cvh_set_image of the same bytes
    (stop norm; one channel: the exact integer sum of squares); the mask, both polarities, is the restatement's and the host form's;
    planes out, both layouts, are the source again.  Then the same as member 1 of 3 of the batch calls."""
    h, w = T.IO_SHAPE
    n = h * w
    assert T.trips(T.IO, h, w) == 2 and n % 16 == 1
    p = capi.make_params(tol=1.0)
    small = [(100, 517, channels), (3, 700, 4 - channels)]
    u0 = np.random.default_rng(11).standard_normal((h, w))
    u0.reshape(-1)[[0, T.first_trip(T.IO, h, w) * 16, n - 1]] = [NAN, -0.0, 1e-60]      # the mask rule at the seams of the second trip
    with capi.Context(h, w, channels, p) as dev, capi.Context(h, w, channels, p) as host:
        for ctx in (dev, host):
            ctx.set_levelset(u0)
        want_mask = {inv: S.mask_of(u0, inv).astype(np.uint8) for inv in (0, 1)}
        single = {}
        for layout in (PLANAR, INTERLEAVED):
            img = rand_image(h, w, channels, 40 + layout + channels)
            planes = planes_of(img)
            dev.set_image_device(hip.upload(source_bytes(img, layout), 1), layout)
            host.set_image(planes)
            assert all(np.array_equal(a, b) for a, b in zip(dev.get_image(), planes)), layout
            stop = dev.get_stop_condition()
            assert stop == host.get_stop_condition(), layout
            if channels == 1:
                assert stop == np.sqrt(np.float64(int((planes[0].astype(np.int64) ** 2).sum())))
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(dev.get_means(), host.get_means()))
            single[layout] = (img, stop)
            for out_layout in (PLANAR, INTERLEAVED):
                d = hip.malloc(n * channels + 64) + 7
                dev.get_image_device(d, out_layout)
                hip.ok(hip.L.hipDeviceSynchronize())
                want = source_bytes(img, out_layout)
                assert np.array_equal(hip.get(d, want.shape, np.uint8), want), (layout, out_layout)
        for inv in (0, 1):
            d = hip.malloc(n + 64) + 1
            dev.get_mask_device(d, inv)
            hip.ok(hip.L.hipDeviceSynchronize())
            got = hip.get(d, (h, w), np.uint8)
            assert np.array_equal(got, want_mask[inv]), inv
            assert np.array_equal(got, dev.get_mask(bool(inv))), inv                   # the host form
        # member 1 of 3
        others = [capi.Context(hh, ww, ch, p) for hh, ww, ch in small]
        try:
            ctxs = [others[0], dev, others[1]]
            imgs_small = [rand_image(hh, ww, ch, 7 + k) for k, (hh, ww, ch) in enumerate(small)]
            for layout in (PLANAR, INTERLEAVED):
                img, stop = single[layout]
                imgs = [imgs_small[0], img, imgs_small[1]]
                dev.set_image([np.zeros((h, w), np.uint8)] * channels)                 # what a batch that skipped the member would leave
                capi.set_image_device_batch(ctxs, [hip.upload(source_bytes(x, layout), off) for x, off in zip(imgs, (3, 1, 0))], layout)
                for ctx, x in zip(ctxs, imgs):
                    assert all(np.array_equal(a, b) for a, b in zip(ctx.get_image(), planes_of(x))), (layout, ctx.h)
                assert dev.get_stop_condition() == stop
            for ctx, (hh, ww, _) in zip(others, small):
                ctx.set_levelset(P.smooth_levelset(hh, ww))
            for inv in (0, 1):
                sinks = [hip.malloc(c.h * c.w + 64) + off for c, off in zip(ctxs, (0, 1, 5))]
                for s, c in zip(sinks, ctxs):
                    hip.put(s, np.full(c.h * c.w, 0xFF, np.uint8))                      # no mask holds 0xFF
                capi.get_mask_device_batch(ctxs, sinks, bool(inv))
                hip.ok(hip.L.hipDeviceSynchronize())
                assert np.array_equal(hip.get(sinks[1], (h, w), np.uint8), want_mask[inv]), inv
                for s, c in ((sinks[0], others[0]), (sinks[2], others[1])):
                    assert np.array_equal(hip.get(s, (c.h, c.w), np.uint8), c.get_mask(bool(inv)))
        finally:
            closing(others)


# ---- histogram, Otsu ----
@pytest.mark.parametrize("channels", [1, 3])
def test_histogram_and_otsu(capi, channels):
    """Random planes and a flat one (every lane of every trip in one bin): histogram, Otsu's threshold and the Otsu start -- whose
    start kernel makes 16 trips at this shape -- against init_util; then as member 1 of 3."""
    h, w = T.IO_SHAPE
    assert T.trips(T.IO, h, w) == 2 and T.trips(T.START, h, w) > 2
    small = [(33, 47, 3), (64, 144, 1)]
    with capi.Context(h, w, channels) as ctx:
        others = [capi.Context(hh, ww, ch) for hh, ww, ch in small]
        try:
            for (hh, ww, ch), c in zip(small, others):
                c.set_image(I.planes_of("random", hh, ww, ch, seed=2))
            own_small = [(c.histogram(), c.init_otsu(2.0, -2.0), c.get_levelset()) for c in others]
            for kind in ("random", "flat"):
                planes = I.planes_of(kind, h, w, channels, seed=1)
                want = I.histogram(planes)
                t = I.otsu(want)
                ctx.set_image(planes)
                hist = ctx.histogram()
                assert np.array_equal(hist, want), kind
                assert int(hist.astype(np.int64).sum()) == h * w
                assert ctx.otsu_threshold() == t == capi.otsu_from_histogram(hist)
                if kind == "flat":
                    assert np.count_nonzero(want) == 1 and t == int(np.flatnonzero(want)[0])
                want_u = I.start_threshold(planes, t, NAN, 0.5)
                assert ctx.init_otsu(NAN, 0.5) == t
                assert np.array_equal(bits(ctx.get_levelset()), bits(want_u)), kind
                # member 1 of 3
                ctxs = [others[0], ctx, others[1]]
                got = capi.histogram_batch(ctxs)
                assert np.array_equal(got[1], hist) and all(np.array_equal(got[k], own_small[j][0]) for k, j in ((0, 0), (2, 1)))
                ctx.init_rect(0, 0, 1, 1)                                             # another level set for the batch to replace
                assert capi.init_otsu_batch(ctxs, 2.0, -2.0) == [own_small[0][1], t, own_small[1][1]]
                assert np.array_equal(bits(ctx.get_levelset()), bits(I.start_threshold(planes, t, 2.0, -2.0))), kind
                for c, own in zip(others, own_small):
                    assert np.array_equal(bits(c.get_levelset()), bits(own[2]))
        finally:
            closing(others)


# ---- the starts: pixel pairs, 526 337 of them for 524 288 lanes, and the odd last pixel ----
def straddling_starts(h, w):
    """a rect and two disks that hold pixels in front of and behind the first pixel of the second trip, and a rect that ends on the
    plane's last (odd) pixel"""
    p2 = 2 * T.first_trip(T.START, h, w)
    row, col = divmod(p2, w)
    assert 3 <= row < h - 3
    rects = [(w // 4, row - 3, w // 2, 6), (5, row, w, h), (col - 2 if col >= 2 else 0, row - 1, 5, 3)]
    disks = [(col, row, 5), (w // 2, row, 40), (w - 1, h - 1, 2)]
    return p2, rects, disks


def both_sides(want, p2, inside):
    """inside and outside pixels both occur in front of and behind flat index p2"""
    m = (bits(want) == bits(np.float64(inside))).reshape(-1)
    return m[:p2].any() and not m[:p2].all() and m[p2:].any() and not m[p2:].all()


@pytest.mark.parametrize("channels", [1, 3])
def test_threshold_start(capi, channels):
    h, w = T.START_SHAPE
    assert T.trips(T.START, h, w) == 2 and (h * w) % 2 == 1
    p2 = 2 * T.first_trip(T.START, h, w)
    B = 255 * channels + 1
    small = [(33, 47, 1), (64, 144, 3)]
    planes = I.planes_of("random", h, w, channels, seed=4)
    with capi.Context(h, w, channels) as ctx:
        others = [capi.Context(hh, ww, ch) for hh, ww, ch in small]
        try:
            ctx.set_image(planes)
            imgs_small = [I.planes_of("random", hh, ww, ch, seed=6) for hh, ww, ch in small]
            for c, x in zip(others, imgs_small):
                c.set_image(x)
            for t, (inside, outside) in ((B // 2, (1.0, -1.0)), (B // 3, (NAN, 2.5)), (0, (-3.0, NAN)), (B - 1, (1.0, 0.0))):
                want = I.start_threshold(planes, t, inside, outside)
                if 0 < t < B - 1:
                    assert both_sides(want, p2, inside)
                ctx.init_threshold(t, inside, outside)
                assert np.array_equal(bits(ctx.get_levelset()), bits(want)), t
                assert ctx.sync()[0] == 0
                ctx.init_rect(0, 0, 1, 1)
                ts = [100, t, 300]
                capi.init_threshold_batch([others[0], ctx, others[1]], ts, inside, outside)
                assert np.array_equal(bits(ctx.get_levelset()), bits(want)), t
                for c, x, tt in zip(others, imgs_small, (ts[0], ts[2])):
                    assert np.array_equal(bits(c.get_levelset()), bits(I.start_threshold(x, tt, inside, outside)))
            assert all(np.array_equal(a, b) for a, b in zip(ctx.get_image(), planes))
        finally:
            closing(others)


def test_rect_and_disk_starts(capi):
    h, w = T.START_SHAPE
    assert T.trips(T.START, h, w) == 2
    p2, rects, disks = straddling_starts(h, w)
    small = [(33, 47, 1), (64, 144, 3)]
    values = [(1.0, 0.0), (NAN, 2.5), (-3.0, NAN)]
    with capi.Context(h, w, 1) as ctx:
        others = [capi.Context(hh, ww, ch) for hh, ww, ch in small]
        try:
            ctxs = [others[0], ctx, others[1]]
            for k, r in enumerate(rects):
                inside, outside = values[k % 3]
                want = I.start_rect(h, w, *r, inside, outside)
                assert both_sides(want, p2, inside), r
                ctx.init_rect(*r, inside, outside)
                assert np.array_equal(bits(ctx.get_levelset()), bits(want)), r
                ctx.init_disk(0, 0, 0)
                rows = [(3, 5, 9, 4), r, (100, 10, 80, 20)]
                capi.init_rect_batch(ctxs, rows, inside, outside)
                assert np.array_equal(bits(ctx.get_levelset()), bits(want)), r
                for c, rr in ((others[0], rows[0]), (others[1], rows[2])):
                    assert np.array_equal(bits(c.get_levelset()), bits(I.start_rect(c.h, c.w, *rr, inside, outside)))
            assert bits(I.start_rect(h, w, *rects[1], 1.0, 0.0))[-1, -1] == bits(np.float64(1.0))     # the odd last pixel is inside one of them
            for k, d in enumerate(disks):
                inside, outside = values[(k + 1) % 3]
                want = I.start_disk(h, w, *d, inside, outside)
                if k < 2:
                    assert both_sides(want, p2, inside), d
                ctx.init_disk(*d, inside, outside)
                assert np.array_equal(bits(ctx.get_levelset()), bits(want)), d
                ctx.init_rect(0, 0, 1, 1)
                rows = [(5, 9, 3), d, (72, 32, 40)]
                capi.init_disk_batch(ctxs, rows, inside, outside)
                assert np.array_equal(bits(ctx.get_levelset()), bits(want)), d
                for c, dd in ((others[0], rows[0]), (others[1], rows[2])):
                    assert np.array_equal(bits(c.get_levelset()), bits(I.start_disk(c.h, c.w, *dd, inside, outside)))
        finally:
            closing(others)


# ---- prolong: two coarse pixels of a row per item, 527 364 items for 524 288 lanes ----
def test_prolong(capi):
    """every coarse value is distinct (its flat index), with NaNs of two payloads, -0.0 and both infinities planted in the items of the
    second trip: a misplaced copy shows wherever it lands"""
    h, w = T.PROLONG_FINE
    hc, wc = P.coarse_shape(h, w)
    assert T.trips(T.PROLONG, h, w) == 2 and h % 2 == 1 and w % 2 == 1
    per_row = T.counts(T.PROLONG, h, w)[0] // hc
    uc = np.arange(hc * wc, dtype=np.float64).reshape(hc, wc)
    b = uc.view(np.uint64)
    t2 = T.first_trip(T.PROLONG, h, w)
    for k, pattern in enumerate(P.SPECIALS[:6]):
        r, p = divmod(t2 + 97 * k, per_row)                  # item t2 + 97 k holds coarse pixels (r, 2p) and (r, 2p + 1)
        b[r, 2 * p + (k & 1)] = pattern
    b[-1, -1] = P.SPECIALS[0]                                 # the last item: one value, one fine row and column of it
    want = P.prolong(uc, h, w)
    small = [(17, 33), (64, 144)]
    coarse_small = [capi.Context(*P.coarse_shape(*s), 1) for s in small]
    fine_small = [capi.Context(*s, 1) for s in small]
    with capi.Context(hc, wc, 1) as coarse, capi.Context(h, w, 1) as fine:
        try:
            coarse.set_levelset(uc)
            coarse.prolong_levelset_to(fine)
            assert np.array_equal(bits(fine.get_levelset()), bits(want))
            assert fine.sync()[0] == 0
            assert np.array_equal(bits(coarse.get_levelset()), bits(uc))
            ucs = [P.special_levelset(*P.coarse_shape(*s), seed=3) for s in small]
            for c, u in zip(coarse_small, ucs):
                c.set_levelset(u)
            fine.init_rect(0, 0, 1, 1)
            capi.prolong_levelset_batch([coarse_small[0], coarse, coarse_small[1]], [fine_small[0], fine, fine_small[1]])
            assert np.array_equal(bits(fine.get_levelset()), bits(want))
            for f, u, s in zip(fine_small, ucs, small):
                assert np.array_equal(bits(f.get_levelset()), bits(P.prolong(u, *s)))
        finally:
            closing(coarse_small + fine_small)


# ---- restrict: 174 764 coarse rows of two 16-pixel runs and a 3-pixel tail, 524 292 items for 524 288 lanes ----
@pytest.mark.parametrize("channels", [1, 3])
def test_restrict(capi, channels):
    h, w = T.RESTRICT_FINE
    hc, wc = P.coarse_shape(h, w)
    assert T.trips(T.RESTRICT, h, w) == 2 and h % 2 == 1 and T.counts(T.RESTRICT, h, w)[0] == 3 * hc
    p = capi.make_params(tol=1.0)
    small = [(31, 50), (33, 257)]
    planes = P.planes_of("random", h, w, channels)
    want = [P.restrict(q) for q in planes]
    fine_small = [capi.Context(*s, channels, p) for s in small]
    coarse_small = [capi.Context(*P.coarse_shape(*s), channels, p) for s in small]
    with capi.Context(h, w, channels, p) as fine, capi.Context(hc, wc, channels, p) as coarse, capi.Context(hc, wc, channels, p) as control:
        try:
            u0 = P.smooth_levelset(hc, wc)
            control.set_image(want)
            control.set_levelset(u0)
            coarse.set_levelset(u0)
            fine.set_image(planes)
            fine.restrict_image_to(coarse)
            assert all(np.array_equal(a, b) for a, b in zip(coarse.get_image(), want))
            stop = coarse.get_stop_condition()
            assert stop == control.get_stop_condition()
            if channels == 1:
                assert stop == np.sqrt(np.float64(int((want[0].astype(np.int64) ** 2).sum())))
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(coarse.get_means(), control.get_means()))
            assert all(np.array_equal(a, b) for a, b in zip(fine.get_image(), planes))
            # member 1 of 3
            imgs = [P.planes_of("random", *s, channels, seed=5) for s in small]
            for f, x in zip(fine_small, imgs):
                f.set_image(x)
            coarse.set_image([np.zeros((hc, wc), np.uint8)] * channels)
            capi.restrict_image_batch([fine_small[0], fine, fine_small[1]], [coarse_small[0], coarse, coarse_small[1]])
            assert all(np.array_equal(a, b) for a, b in zip(coarse.get_image(), want))
            assert coarse.get_stop_condition() == stop
            for c, x in zip(coarse_small, imgs):
                assert all(np.array_equal(a, P.restrict(q)) for a, q in zip(c.get_image(), x))
        finally:
            closing(fine_small + coarse_small)


# ---- the energy: 514 item rows for the 256 lanes of the reduce stage; 8193 items for the 8192 waves of the term stage ----
def wavy_levelset(h, w):
    """both signs in every item, |u| < 4: no item's share of a term is negligible"""
    ii, jj = np.mgrid[0:h, 0:w]
    return 3.0 * np.sin(0.37 * ii + 0.11) * np.cos(0.91 * jj) + 0.2


ENERGY_CASES = [T.ENERGY_REDUCE_SHAPE + (1,), T.ENERGY_REDUCE_SHAPE + (3,), T.ENERGY_TERMS_SHAPE + (1,)]


def energy_context(capi, h, w, channels, seed=0):
    ctx = capi.Context(h, w, channels, capi.make_params(**params_of(channels)))
    ctx.set_image(E.planes_of("random", h, w, channels, seed=seed))
    return ctx


@pytest.mark.parametrize("h,w,channels", ENERGY_CASES)
def test_energy_terms_match_the_restatement(capi, h, w, channels):
    assert T.trips(T.ENERGY_REDUCE, h, w) >= 2
    assert T.trips(T.ENERGY_TERMS, h, w) == (2 if (h, w) == T.ENERGY_TERMS_SHAPE else 1)
    pk = params_of(channels)
    planes = E.planes_of("random", h, w, channels)
    with energy_context(capi, h, w, channels) as ctx:
        for name, u in (("smooth", E.smooth_levelset(h, w)), ("wavy", wavy_levelset(h, w))):
            ctx.set_levelset(u)
            e = ctx.energy()
            c1, c2 = ctx.get_means()
            assert np.array_equal(bits(e.c1), bits(c1)) and np.array_equal(bits(e.c2), bits(c2)), (name, e, c1, c2)
            assert same_bits(ctx.energy(), e), name
            check_terms(e, restated(ctx, planes, u, pk, e), f"{h}x{w}x{channels} {name}")
        u = E.inf_levelset(h, w)                                   # non-finite exactly where the restatement is
        ctx.set_levelset(u)
        e = ctx.energy()
        check_terms(e, restated(ctx, planes, u, pk, e), f"{h}x{w}x{channels} infinities")


@pytest.mark.parametrize("h,w,channels", ENERGY_CASES)
def test_energy_constant_inputs_give_exact_terms(capi, h, w, channels):
    """u = 0 adds 0.5 per pixel and planes of zeros add 0.0: exact in any order, so a skipped or repeated item shows bit for bit"""
    pk = params_of(channels)
    with capi.Context(h, w, channels, capi.make_params(**pk)) as ctx:
        ctx.set_image(E.planes_of("all0", h, w, channels))
        ctx.set_levelset(np.zeros((h, w)))
        e = ctx.energy()
        zeros = (0.0,) * channels
        assert e.length == 0.0 and e.area == h * w / 2 and tuple(e.fit_in) == zeros and tuple(e.fit_out) == zeros
        assert e.total == pk.get("mu", 0.5) * 0.0 + pk.get("nu", 0.0) * (h * w / 2) + (1.0 / channels) * 0.0
        ctx.set_levelset(np.full((h, w), -2.5))
        assert ctx.energy().length == 0.0


def test_energy_batch_members_equal_their_single_calls(capi):
    """the reduce-capped member (three channels) and the term-capped one, each as member 1 of 3 behind a small member"""
    (h1, w1), (h2, w2) = T.ENERGY_REDUCE_SHAPE, T.ENERGY_TERMS_SHAPE
    ctxs = [energy_context(capi, 33, 257, 3, seed=1), energy_context(capi, h1, w1, 3, seed=2), energy_context(capi, h2, w2, 1, seed=3)]
    try:
        ctxs[0].set_levelset(E.smooth_levelset(33, 257))
        ctxs[1].set_levelset(wavy_levelset(h1, w1))
        ctxs[2].set_levelset(wavy_levelset(h2, w2))
        alone = [c.energy() for c in ctxs]
        a = capi.energy_batch(ctxs)
        b = capi.energy_batch([ctxs[0], ctxs[2], ctxs[1]])
        assert all(same_bits(x, y) for x, y in zip(a, alone)), (a, alone)
        assert all(same_bits(x, y) for x, y in zip(b, [alone[0], alone[2], alone[1]])), (b, alone)
    finally:
        closing(ctxs)


# ---- score, row stage: a workgroup owns rows r, r + 8192 (, r + 16384) for r < 3 ----
def score_planes(h, w):
    """(mask M, truth T): one-row-high segments -- every pixel of them is a surface pixel -- placed so that
      (i)   rows r and r + 8192 of a workgroup both hold surface pixels of both sets (r = 0, 2);
      (ii)  a row with many surface pixels (the whole row) is followed in its workgroup by a row with none or by one with few: rows 0 /
            8192 (/ 16384: few again behind an empty row 8192 where the plane has three rows per workgroup) and 2 / 8194 the other way round;
      (iii) the lone pixels in the middle of the plane have their column's nearest pixel of the other surface more than 100 bands above
            and below them."""
    m, t = np.zeros((h, w), bool), np.zeros((h, w), bool)
    half, last = w // 2, h - 1
    three = h > 2 * 8192
    m[0, :half + 1], t[0, half:] = True, True                    # many
    if three:
        m[16384, 1], t[16384, w - 2], t[16384, 0] = True, True, True     # few, behind the empty row 8192
    else:
        m[8192, 1], t[8192, w - 2] = True, True                  # few
    m[1, 0], t[8193, w - 1], t[8193, half + 1] = True, True, True    # rows of one surface each
    m[2, w - 1], t[2, 0] = True, True                            # few, then many
    m[8194, half - 1:], t[8194, :half] = True, True
    mid = (8194 // 2) if not three else 4097
    m[mid, half + 1], t[mid + 4, half - 2] = True, True          # M's lone pixel sits in a column of T's rows 0 / 8194 only, and T's likewise
    if three:
        m[last, :], t[last - 1, ::7] = True, True
    return m, t


@pytest.mark.parametrize("h,w", T.ROW_SHAPES + [T.SCORE_THREE_ROWS])
def test_score(capi, hip, h, w):
    assert T.trips(T.ROWS, h, w) == (3 if (h, w) == T.SCORE_THREE_ROWS else 2)
    m, t = score_planes(h, w)
    sm, st = S.surface(m), S.surface(t)
    assert all(sm[r].any() and st[r].any() for r in (0, 2, 8194)) and (not sm[8193].any()) and not st[1].any()
    mid = np.flatnonzero(sm[:, w // 2 + 1])                       # (iii): the column of M's lone pixel, in surf(T)
    col_t = np.flatnonzero(st[:, w // 2 + 1])
    lone = [r for r in mid if 3300 < r < 4200][0]
    assert (np.abs(col_t - lone) > 100 * 32).all() and (col_t < lone).any() and (col_t > lone).any()
    truth = t.astype(np.uint8) * 255
    d_truth = hip.upload(truth, offset=3)
    L = capi.lib()
    with capi.Context(h, w, 1) as ctx:
        ctx.set_levelset(S.levelset_of(m, np.random.default_rng(8)))
        for invert in (False, True):
            want = S.score(m != invert, t, 4)
            assert want["defined"] == 1
            got = ctx.score(d_truth, invert=invert, tol=2.0)
            assert S.as_dict(got) == want, (invert, {k: (v, want[k]) for k, v in S.as_dict(got).items() if v != want[k]})
            a, b = capi.MaskScore(), capi.MaskScore()              # the host form, raw bytes
            assert L.cvh_score_mask(ctx._h, truth.ctypes.data_as(C.POINTER(C.c_uint8)), int(invert), 4, C.byref(a)) == 0
            assert L.cvh_score_mask_device(ctx._h, d_truth, int(invert), 4, C.byref(b), None) == 0
            assert bytes(a) == bytes(b)


def test_score_batch_members_equal_their_single_calls(capi, hip):
    shapes = [(33, 257)] + T.ROW_SHAPES
    ctxs, truths, planes = [], [], []
    try:
        for h, w in shapes:
            m, t = score_planes(h, w) if h > 8192 else (S.mask_of(S.case("disks", h, w)[0]), S.case("disks", h, w)[1] != 0)
            ctx = capi.Context(h, w, 1)
            ctxs.append(ctx)
            ctx.set_levelset(S.levelset_of(m))
            truths.append(hip.upload(t.astype(np.uint8), offset=len(ctxs)))
            planes.append((m, t))
        for invert in (False, True):
            alone = [c.score(d, invert=invert) for c, d in zip(ctxs, truths)]
            for order in ([0, 1, 2], [0, 2, 1]):
                got = capi.score_batch([ctxs[k] for k in order], [truths[k] for k in order], invert=invert)
                assert got == [alone[k] for k in order], (invert, order)
            for s, (m, t) in zip(alone, planes):
                assert S.as_dict(s) == S.score(m != invert, t, 4)
    finally:
        closing(ctxs)


# ---- reinit, row stage, with a real row search ----
@pytest.mark.parametrize("kind", ["special", "rectangle"])
def test_reinit(capi, kind):
    h, w = T.ROW_SHAPES[0]
    assert T.trips(T.ROWS, h, w) == 2 and w > 1
    with capi.Context(h, w, 1) as ctx, capi.Context(40, 300, 1) as a, capi.Context(100, 517, 1) as b:
        for c in (ctx, a, b):
            give_levelset(c, kind, c.h, c.w)
        before = [c.get_levelset() for c in (ctx, a, b)]
        d2, want, changed = R.signed_edt(before[0])
        assert changed and ctx.reinit() is True
        got = ctx.get_levelset()
        print(f"{h}x{w} {kind}: max d2={int(d2.max())} differing={int((bits(got) != bits(want)).sum())}")
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(ctx.get_mask().astype(bool), R.mask_of(before[0]))
        ctx.set_levelset(before[0])
        assert capi.reinit_batch([a, ctx, b]) == [True, True, True]
        assert np.array_equal(bits(ctx.get_levelset()), bits(want))
        for c, u in ((a, before[1]), (b, before[2])):
            assert np.array_equal(bits(c.get_levelset()), bits(R.signed_edt(u)[1]))
