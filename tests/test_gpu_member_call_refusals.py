"""The four calls that replace a context's planes on the device (cvh_set_image_device*, cvh_convert_colour*, cvh_luma_image*,
cvh_restrict_image*) and the two checks of "n pairs of contexts" (the colour pairs', the pyramid pairs' -- cvh_prolong_levelset* shares
the latter): the FULL text of every refusal, which refusal wins when two faults meet, and one positive case per plane-writing call.

The expected texts are written out here; none is produced by the library.  A refusal's text is what cvh_last_error(NULL) holds and,
where the library records it there, what the call's member 0 holds (a pair call's member 0 is pair 0's DESTINATION; an empty list and
a NULL entry of a pair list are recorded for no context); the return code is the stated one; and every context is as it was: the
planes, the step count cvh_sync reports, and a context without an image still refuses cvh_run for that.

Contexts are 16 x 16, 16 x 25 and 32 x 50 with one and three channels (the positive restrict case adds the 64 x 99 fine context whose
coarse one is 32 x 50).  NOT covered: "is too large, h * w must stay below 2^32" (needs planes of 2^32 pixels) and "is on device %d"
(needs a second GPU).  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import colour_util as CU
import pyramid_util as PU
import test_gpu_device_io as DIO

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, 1, 3
NO_IMAGE = "no image set (call cvh_set_image first)"
STEPS = 3
# name: (h, w, channels, holds an image and a level set STEPS iterations old)
CONTEXTS = {"A3": (16, 25, 3, True), "B3": (32, 50, 3, True), "S3": (16, 16, 3, True), "E3": (16, 25, 3, False), "F3": (32, 50, 3, False),
            "A1": (16, 25, 1, True), "B1": (32, 50, 1, True), "S1": (16, 16, 1, True), "E1": (16, 25, 1, False)}


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def image_of(name):
    h, w, ch, _ = CONTEXTS[name]
    return DIO.planes_of(DIO.rand_image(h, w, ch, seed=sum(map(ord, name))))


@pytest.fixture(scope="module")
def K(capi):
    """the contexts of CONTEXTS, by name"""
    ctxs = {name: capi.Context(h, w, ch, capi.make_params(tol=0.0)) for name, (h, w, ch, _) in CONTEXTS.items()}
    for name, c in ctxs.items():
        if CONTEXTS[name][3]:
            c.set_image(image_of(name))
            c.init_checkerboard()
            c.enqueue_steps(STEPS)
            assert c.sync()[0] == STEPS
    yield ctxs
    for c in ctxs.values():
        c.close()


def members(K, names):
    """a ctypes list of handles; a name of None is a NULL entry"""
    return (C.c_void_p * max(len(names), 1))(*[K[n]._h.value if n else None for n in names])


ADDR = (C.c_void_p * 3)(64, 64, 64)   # device "pointers" of calls refused before any pointer is looked at


def ingest(names, ptrs=ADDR, layout=0):
    return lambda L, K: L.cvh_set_image_device_batch(members(K, names), len(names), ptrs, layout, None)


def convert(names, space=1, order=0, inverse=0):
    return lambda L, K: L.cvh_convert_colour_batch(members(K, names), len(names), space, order, inverse)


def luma(srcs, dsts, order=0):
    return lambda L, K: L.cvh_luma_image_batch(members(K, srcs), members(K, dsts), len(srcs), order)


def restrict(fines, coarses):
    return lambda L, K: L.cvh_restrict_image_batch(members(K, fines), members(K, coarses), len(fines))


def prolong(coarses, fines):
    return lambda L, K: L.cvh_prolong_levelset_batch(members(K, coarses), members(K, fines), len(fines))


ONCE = " (a context may be listed once)"
# (id, call, return code, text, the context that also holds the text or None)
REFUSALS = [
    # ---- an empty list ----
    ("ingest-empty", lambda L, K: L.cvh_set_image_device_batch(None, 0, None, 0, None), ERR_ARG,
     "cvh_set_image_device_batch: empty member list (ctxs = (nil), n = 0)", None),
    ("convert-empty", lambda L, K: L.cvh_convert_colour_batch(None, 0, 1, 0, 0), ERR_ARG,
     "cvh_convert_colour_batch: empty member list (ctxs = (nil), n = 0)", None),
    ("luma-empty", lambda L, K: L.cvh_luma_image_batch(None, None, 0, 0), ERR_ARG,
     "cvh_luma_image_batch: empty pair list (srcs = (nil), dsts = (nil), n = 0)", None),
    ("restrict-empty", lambda L, K: L.cvh_restrict_image_batch(None, None, 0), ERR_ARG,
     "cvh_restrict_image_batch: empty pair list (fines = (nil), coarses = (nil), n = 0)", None),
    ("prolong-empty", lambda L, K: L.cvh_prolong_levelset_batch(None, None, 0), ERR_ARG,
     "cvh_prolong_levelset_batch: empty pair list (fines = (nil), coarses = (nil), n = 0)", None),
    # ---- a NULL entry in each list ----
    ("ingest-null", ingest(["A3", None]), ERR_ARG, "cvh_set_image_device_batch: member 1 is NULL", "A3"),
    ("convert-null", convert(["A3", None]), ERR_ARG, "cvh_convert_colour_batch: member 1 is NULL", "A3"),
    ("convert-null-single", lambda L, K: L.cvh_convert_colour(None, 1, 0, 0), ERR_ARG, "cvh_convert_colour: member 0 is NULL", None),
    ("luma-null-src", luma(["A3", None], ["A1", "E1"]), ERR_ARG, "cvh_luma_image_batch: pair 1: the source context is NULL", None),
    ("luma-null-dst", luma(["A3", "B3"], ["A1", None]), ERR_ARG, "cvh_luma_image_batch: pair 1: the destination context is NULL", None),
    ("luma-null-both", luma([None], [None]), ERR_ARG, "cvh_luma_image_batch: pair 0: the source context is NULL", None),
    ("restrict-null-fine", restrict(["B3", None], ["A3", "E3"]), ERR_ARG, "cvh_restrict_image_batch: pair 1: the fine context is NULL", None),
    ("restrict-null-coarse", restrict(["B3", "F3"], ["A3", None]), ERR_ARG, "cvh_restrict_image_batch: pair 1: the coarse context is NULL", None),
    ("restrict-null-both", restrict([None], [None]), ERR_ARG, "cvh_restrict_image_batch: pair 0: the fine context is NULL", None),
    ("prolong-null-coarse", prolong(["A3", None], ["B3", "F3"]), ERR_ARG, "cvh_prolong_levelset_batch: pair 1: the coarse context is NULL", None),
    ("prolong-null-fine", prolong(["A3", "E3"], ["B3", None]), ERR_ARG, "cvh_prolong_levelset_batch: pair 1: the fine context is NULL", None),
    # ---- a context twice in one list, and once in each list ----
    ("ingest-twice", ingest(["A3", "B3", "A3"]), ERR_ARG, "cvh_set_image_device_batch: member 2 duplicates member 0", "A3"),
    ("convert-twice", convert(["A3", "B3", "A3"]), ERR_ARG, "cvh_convert_colour_batch: member 2 duplicates member 0", "A3"),
    ("luma-src-twice", luma(["A3", "A3"], ["A1", "E1"]), ERR_ARG,
     "cvh_luma_image_batch: pair 1: its source context is also pair 0's source context" + ONCE, "A1"),
    ("luma-dst-twice", luma(["A3", "E3"], ["A1", "A1"]), ERR_ARG,
     "cvh_luma_image_batch: pair 1: its destination context is also pair 0's destination context" + ONCE, "A1"),
    ("luma-both-lists", lambda L, K: L.cvh_luma_image(K["A3"]._h, K["A3"]._h, 0), ERR_ARG,
     "cvh_luma_image: pair 0: its source context is also pair 0's destination context" + ONCE, "A3"),
    ("luma-across-pairs", luma(["A3", "E3"], ["A1", "A3"]), ERR_ARG,
     "cvh_luma_image_batch: pair 0: its source context is also pair 1's destination context" + ONCE, "A1"),
    ("restrict-fine-twice", restrict(["B3", "B3"], ["A3", "E3"]), ERR_ARG,
     "cvh_restrict_image_batch: pair 1: its fine context is also pair 0's fine context" + ONCE, "A3"),
    ("restrict-coarse-twice", restrict(["B3", "F3"], ["A3", "A3"]), ERR_ARG,
     "cvh_restrict_image_batch: pair 1: its coarse context is also pair 0's coarse context" + ONCE, "A3"),
    ("restrict-both-lists", lambda L, K: L.cvh_restrict_image(K["B3"]._h, K["B3"]._h), ERR_ARG,
     "cvh_restrict_image: pair 0: its fine context is also pair 0's coarse context" + ONCE, "B3"),
    ("prolong-both-lists", lambda L, K: L.cvh_prolong_levelset(K["A3"]._h, K["A3"]._h), ERR_ARG,
     "cvh_prolong_levelset: pair 0: its coarse context is also pair 0's fine context" + ONCE, "A3"),
    ("prolong-coarse-twice", prolong(["A3", "A3"], ["B3", "F3"]), ERR_ARG,
     "cvh_prolong_levelset_batch: pair 1: its coarse context is also pair 0's coarse context" + ONCE, "B3"),
    # ---- the channel rules ----
    ("convert-channels", convert(["A3", "A1"]), ERR_ARG, "cvh_convert_colour_batch: member 1 has 1 channel(s), a colour conversion takes 3", "A3"),
    ("luma-src-channels", lambda L, K: L.cvh_luma_image(K["A1"]._h, K["E1"]._h, 0), ERR_ARG,
     "cvh_luma_image: pair 0: the source context has 1 channel(s), a luma plane is taken from 3", "E1"),
    ("luma-dst-channels", lambda L, K: L.cvh_luma_image(K["A3"]._h, K["E3"]._h, 0), ERR_ARG,
     "cvh_luma_image: pair 0: the destination context has 3 channels, a luma plane goes into 1", "E3"),
    ("restrict-channels", lambda L, K: L.cvh_restrict_image(K["B3"]._h, K["A1"]._h), ERR_ARG,
     "cvh_restrict_image: pair 0: the fine context has 3 channel(s), the coarse one 1", "A1"),
    # ---- the shape rules ----
    ("luma-shape", luma(["A3", "B3"], ["A1", "S1"]), ERR_ARG,
     "cvh_luma_image_batch: pair 1: the destination of a 32 x 50 source must be 32 x 50 too, got 16 x 16", "A1"),
    ("restrict-shape", lambda L, K: L.cvh_restrict_image(K["B3"]._h, K["S3"]._h), ERR_ARG,
     "cvh_restrict_image: pair 0: the coarse context of a 32 x 50 plane must be 16 x 25, got 16 x 16", "S3"),
    ("prolong-shape", prolong(["A1", "S3"], ["B1", "B3"]), ERR_ARG,
     "cvh_prolong_levelset_batch: pair 1: the coarse context of a 32 x 50 plane must be 16 x 25, got 16 x 16", "B1"),
    # ---- a bad space, order, inverse and layout; a NULL pointer list and a NULL pointer ----
    ("convert-space", lambda L, K: L.cvh_convert_colour(K["A3"]._h, 0, 0, 0), ERR_ARG,
     "cvh_convert_colour: space must be CVH_COLOUR_YCRCB (1) or CVH_COLOUR_YUV (2), got 0", "A3"),
    ("convert-order", lambda L, K: L.cvh_convert_colour(K["A3"]._h, 2, 2, 0), ERR_ARG,
     "cvh_convert_colour: order must be CVH_ORDER_BGR (0) or CVH_ORDER_RGB (1), got 2", "A3"),
    ("convert-inverse", lambda L, K: L.cvh_convert_colour(K["A3"]._h, 2, 1, 2), ERR_ARG, "cvh_convert_colour: inverse must be 0 or 1, got 2", "A3"),
    ("luma-order", lambda L, K: L.cvh_luma_image(K["A3"]._h, K["A1"]._h, -1), ERR_ARG,
     "cvh_luma_image: order must be CVH_ORDER_BGR (0) or CVH_ORDER_RGB (1), got -1", "A1"),
    ("ingest-layout", lambda L, K: L.cvh_set_image_device(K["A3"]._h, 64, 2, None), ERR_ARG,
     "cvh_set_image_device: layout must be CVH_LAYOUT_PLANAR (0) or CVH_LAYOUT_INTERLEAVED (1), got 2", "A3"),
    ("ingest-pointer-list", ingest(["A3", "B1"], ptrs=None), ERR_ARG, "cvh_set_image_device_batch: the list of device pointers is NULL", "A3"),
    ("ingest-pointer", lambda L, K: L.cvh_set_image_device(K["A3"]._h, None, 0, None), ERR_ARG,
     "cvh_set_image_device: member 0: the device pointer is NULL", "A3"),
    # ---- a member without an image, a coarse context without a level set ----
    ("convert-no-image", convert(["A3", "E3"]), ERR_STATE, "cvh_convert_colour_batch: member 1 has no image (call cvh_set_image first)", "A3"),
    ("luma-no-image", luma(["A3", "E3"], ["A1", "E1"]), ERR_STATE,
     "cvh_luma_image_batch: pair 1: the source context has no image (call cvh_set_image first)", "A1"),
    ("restrict-no-image", lambda L, K: L.cvh_restrict_image(K["F3"]._h, K["A3"]._h), ERR_STATE,
     "cvh_restrict_image: pair 0: the fine context has no image (call cvh_set_image first)", "A3"),
    ("prolong-no-levelset", lambda L, K: L.cvh_prolong_levelset(K["E3"]._h, K["B3"]._h), ERR_STATE,
     "cvh_prolong_levelset: pair 0: the coarse context has no level set", "B3"),
    # ---- two faults at once: which one is reported ----
    ("convert-space-before-channels", convert(["A3", "A1"], space=3), ERR_ARG,
     "cvh_convert_colour_batch: space must be CVH_COLOUR_YCRCB (1) or CVH_COLOUR_YUV (2), got 3", "A3"),
    ("luma-listed-once-before-order", luma(["A3", "A3"], ["A1", "E1"], order=2), ERR_ARG,
     "cvh_luma_image_batch: pair 1: its source context is also pair 0's source context" + ONCE, "A1"),
    ("ingest-pointer-list-before-layout", ingest(["A3", "B1"], ptrs=None, layout=2), ERR_ARG,
     "cvh_set_image_device_batch: the list of device pointers is NULL", "A3"),
    ("restrict-shape-before-no-image", restrict(["F3", "B3"], ["A3", "S3"]), ERR_ARG,
     "cvh_restrict_image_batch: pair 1: the coarse context of a 32 x 50 plane must be 16 x 25, got 16 x 16", "A3"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_text_code_and_untouched_contexts(capi, K, case):
    _, call, code, text, holder = case
    L = capi.lib()
    rc = call(L, K)
    got = L.cvh_last_error(None).decode()
    print(rc, repr(got))
    assert got == text
    assert rc == code
    if holder:
        assert L.cvh_last_error(K[holder]._h).decode() == text
    for name, c in K.items():
        if CONTEXTS[name][3]:
            assert all(np.array_equal(a, b) for a, b in zip(c.get_image(), image_of(name))), name
            assert c.sync()[0] == STEPS, name
        else:
            with pytest.raises(capi.CvhError) as e:
                c.run(1)
            assert e.value.code == ERR_STATE and str(e.value).endswith(NO_IMAGE), name


# ---- one positive case per plane-writing call: two members, 16 x 25 and 32 x 50 ----

def as_set_image_leaves_them(capi, written):
    """each written context against a fresh one given the same bytes through set_image: the image, the stop condition and the means of
    the same level set, doubles compared as bit patterns"""
    for c in written:
        planes = c.get_image()
        with capi.Context(c.h, c.w, c.channels) as fresh:
            fresh.set_image(planes)
            assert all(np.array_equal(a, b) for a, b in zip(fresh.get_image(), planes))
            for x in (c, fresh):
                x.set_levelset(PU.smooth_levelset(c.h, c.w))
            assert c.get_stop_condition() == fresh.get_stop_condition()
            for a, b in zip(c.get_means(), fresh.get_means()):
                assert np.array_equal(PU.bits(a), PU.bits(b))


def test_ingest_of_two_shapes_leaves_what_set_image_leaves(capi):
    hip = DIO.Hip()
    try:
        imgs = [DIO.rand_image(16, 25, 3, seed=1), DIO.rand_image(32, 50, 1, seed=2)]
        with capi.Context(16, 25, 3) as a, capi.Context(32, 50, 1) as b:
            capi.set_image_device_batch([a, b], [hip.upload(DIO.source_bytes(i, DIO.PLANAR)) for i in imgs])
            for c, img in zip((a, b), imgs):
                assert all(np.array_equal(x, y) for x, y in zip(c.get_image(), DIO.planes_of(img)))
            as_set_image_leaves_them(capi, [a, b])
    finally:
        hip.free_all()


def test_convert_of_two_shapes_leaves_what_set_image_leaves(capi):
    imgs = [CU.planes_of("random", 16, 25, seed=3), CU.planes_of("random", 32, 50, seed=4)]
    with capi.Context(16, 25, 3) as a, capi.Context(32, 50, 3) as b:
        for c, img in zip((a, b), imgs):
            c.set_image(img)
        capi.convert_colour_batch([a, b], "ycrcb", "bgr")
        for c, img in zip((a, b), imgs):
            assert all(np.array_equal(x, y) for x, y in zip(c.get_image(), CU.forward(img, "ycrcb", "bgr")))
        as_set_image_leaves_them(capi, [a, b])


def test_luma_of_two_shapes_leaves_what_set_image_leaves(capi):
    imgs = [CU.planes_of("random", 16, 25, seed=5), CU.planes_of("random", 32, 50, seed=6)]
    with capi.Context(16, 25, 3) as a, capi.Context(32, 50, 3) as b, capi.Context(16, 25, 1) as da, capi.Context(32, 50, 1) as db:
        for c, img in zip((a, b), imgs):
            c.set_image(img)
        capi.luma_image_batch([a, b], [da, db], "bgr")
        for s, d, img in zip((a, b), (da, db), imgs):
            assert np.array_equal(d.get_image()[0], CU.luma(img, "bgr"))
            assert all(np.array_equal(x, y) for x, y in zip(s.get_image(), img))   # the sources are only read
        as_set_image_leaves_them(capi, [da, db])


def test_restrict_of_two_shapes_leaves_what_set_image_leaves(capi):
    imgs = [PU.planes_of("random", 32, 50, 3, seed=7), PU.planes_of("random", 64, 99, 1, seed=8)]
    with capi.Context(32, 50, 3) as fa, capi.Context(64, 99, 1) as fb, capi.Context(16, 25, 3) as ca, capi.Context(32, 50, 1) as cb:
        for c, img in zip((fa, fb), imgs):
            c.set_image(img)
        capi.restrict_image_batch([fa, fb], [ca, cb])
        for f, c, img in zip((fa, fb), (ca, cb), imgs):
            assert all(np.array_equal(x, PU.restrict(y)) for x, y in zip(c.get_image(), img))
            assert all(np.array_equal(x, y) for x, y in zip(f.get_image(), img))   # the fine contexts are only read
        as_set_image_leaves_them(capi, [ca, cb])
