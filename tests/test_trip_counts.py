"""The member-table kernels loop behind a cap on a member's workgroups (2048 for most, 8192 row workgroups for reinit and score; the
energy's reduce stage adds item rows 256 at a time).  This file pins, on the CPU and from the library's own block functions
(trips_util.counts), which shapes reach those loops: every case of test_gpu_second_trips.py makes a second trip, every shape of the
older lists makes exactly one -- the gap that file closes --, and the 4096 x 4096 workload of BASELINE.md makes the trips DESIGN.md 4.3
names.  Moving a cap fails here instead of silently returning the GPU cases to one trip."""
import pytest

import init_util
import pyramid_util
import score_util
import trips_util as T
from test_gpu_device_io import SHAPES as IO_SHAPES
from test_gpu_reinit import SHAPES as REINIT_SHAPES

NAMES = {T.IO: "io", T.START: "start", T.RESTRICT: "restrict", T.PROLONG: "prolong", T.ENERGY_TERMS: "energy terms",
         T.ENERGY_REDUCE: "energy reduce", T.ROWS: "rows", T.COLUMNS: "columns"}


@pytest.mark.parametrize("op,shape", T.CASES, ids=lambda v: NAMES[v] if isinstance(v, int) else f"{v[0]}x{v[1]}")
def test_every_new_case_makes_a_second_trip(op, shape):
    items, nblk, takers = T.counts(op, *shape)
    print(NAMES[op], shape, "items", items, "workgroups", nblk, "per workgroup and trip", takers)
    assert items > nblk * takers
    assert T.trips(op, *shape) >= 2


def test_the_caps_are_where_the_shapes_were_derived_for():
    """the shapes are the smallest that pass: 2048 workgroups of 256 lanes, 2048 of four waves, 8192 row workgroups, 256 reduce lanes"""
    for op, shape in ((T.IO, T.IO_SHAPE), (T.START, T.START_SHAPE), (T.RESTRICT, T.RESTRICT_FINE), (T.PROLONG, T.PROLONG_FINE)):
        assert T.first_trip(op, *shape) == 2048 * 256, (NAMES[op], T.counts(op, *shape))
    assert T.counts(T.IO, *T.IO_SHAPE)[0] == 524672 and (T.IO_SHAPE[0] * T.IO_SHAPE[1]) % 16 == 1
    assert T.counts(T.START, *T.START_SHAPE)[0] == 526337 and (T.START_SHAPE[0] * T.START_SHAPE[1]) % 2 == 1
    assert T.counts(T.PROLONG, *T.PROLONG_FINE)[0] == 527364
    assert T.counts(T.RESTRICT, *T.RESTRICT_FINE)[0] == 524292
    assert T.counts(T.ENERGY_REDUCE, *T.ENERGY_REDUCE_SHAPE) == (514, 1, 256)
    assert T.counts(T.ENERGY_TERMS, *T.ENERGY_REDUCE_SHAPE)[0] == 514 and T.trips(T.ENERGY_TERMS, *T.ENERGY_REDUCE_SHAPE) == 1
    assert T.counts(T.ENERGY_TERMS, *T.ENERGY_TERMS_SHAPE) == (8193, 2048, 4)
    for h, w in T.ROW_SHAPES:
        assert T.counts(T.ROWS, h, w) == (h, 8192, 1) and T.trips(T.ROWS, h, w) == 2
    assert T.trips(T.ROWS, *T.SCORE_THREE_ROWS) == 3
    # the column launches of reinit and score have no cap: a workgroup per band and 256 columns, however tall the plane
    for h, w in T.ROW_SHAPES + [T.SCORE_THREE_ROWS, (65535, 1)]:
        assert T.trips(T.COLUMNS, h, w) == 1


OLD = [("pyramid_util.SHAPES", pyramid_util.SHAPES, (T.RESTRICT, T.PROLONG, T.ENERGY_TERMS, T.ENERGY_REDUCE)),
       ("the energy's 512 x 512 run", [(512, 512)], (T.ENERGY_TERMS, T.ENERGY_REDUCE)),
       ("score_util.SHAPES", score_util.SHAPES, (T.ROWS, T.COLUMNS)),
       ("init_util.SHAPES and the flat megapixel", init_util.SHAPES + [(1024, 1024)], (T.IO, T.START)),
       ("test_gpu_device_io.SHAPES", IO_SHAPES, (T.IO,)),
       ("test_gpu_reinit.SHAPES", REINIT_SHAPES, (T.ROWS, T.COLUMNS))]


@pytest.mark.parametrize("name,shapes,ops", OLD, ids=[o[0] for o in OLD])
def test_the_older_lists_make_one_trip(name, shapes, ops):
    for op in ops:
        for h, w in shapes:
            assert T.trips(op, h, w) == 1, (name, NAMES[op], (h, w), T.counts(op, h, w))
    # the one megapixel start is exactly full: 524 288 pairs for 524 288 lanes
    if (1024, 1024) in shapes and T.START in ops:
        items, nblk, takers = T.counts(T.START, 1024, 1024)
        assert items == nblk * takers == 524288


def test_the_trips_of_the_4096_workload():
    """BASELINE.md's workload: what DESIGN.md 4.3 says of it is what the library reports"""
    got = {NAMES[op]: T.trips(op, 4096, 4096) for op in (T.PROLONG, T.START, T.IO, T.ENERGY_REDUCE)}
    assert got == {"prolong": 4, "start": 16, "io": 2, "energy reduce": 16}


def test_bad_arguments_are_refused():
    import ctypes as C
    from chan_vese_amd import capi
    fn = C.CDLL(capi.LIB_PATH).cvh_debug_trip_counts
    items, nblk, takers = C.c_ulonglong(), C.c_uint(), C.c_uint()
    out = (C.byref(items), C.byref(nblk), C.byref(takers))
    assert fn(-1, 4, 4, *out) == 1 and fn(8, 4, 4, *out) == 1 and fn(0, 0, 4, *out) == 1 and fn(0, 4, 0, *out) == 1
    assert fn(0, 4, 4, None, out[1], out[2]) == 1
