"""How many trips the lanes, waves or workgroups of a member-table kernel make over a member of a given shape -- read from the library
(the diagnostic export cvh_debug_trip_counts, which calls the functions the host units size a member's grid section with; no device
needed), never from a formula restated here -- and the shapes test_gpu_second_trips.py runs: for every operation the smallest plane that
passes the operation's cap with its ragged tail alive.  Shared by test_trip_counts.py (CPU) and test_gpu_second_trips.py."""
import ctypes as C

# the operation codes of cvh_debug_trip_counts (debug_exports.hip)
IO, START, RESTRICT, PROLONG, ENERGY_TERMS, ENERGY_REDUCE, ROWS, COLUMNS = range(8)

# (h, w) of the capped member; for restrict and prolong the FINE grid, as the library's block functions take it
IO_SHAPE = (2049, 4097)             # ingest, image out, mask, histogram: 524 672 pieces and one last pixel
START_SHAPE = (1025, 1027)          # threshold / rect / disk starts: 526 337 pairs and the odd last pixel
PROLONG_FINE = (2051, 2053)         # coarse 1026 x 1027: 527 364 items, odd fine height and width (both drops)
RESTRICT_FINE = (349527, 70)        # coarse 174764 x 35: two 16-pixel runs and a 3-pixel tail per row, the clamped last row
ENERGY_REDUCE_SHAPE = (8193, 129)   # 257 bands x 2 pieces: the second piece one column wide, the last band one row
ENERGY_TERMS_SHAPE = (262145, 3)    # 8193 items for 8192 waves
ROW_SHAPES = [(8195, 5), (8195, 300)]   # reinit (the first) and score (both): rows 0 .. 2 share a workgroup with rows 8192 .. 8194
SCORE_THREE_ROWS = (16387, 300)     # score: a workgroup owns rows r, r + 8192 and r + 16384 for r < 3

# every case of test_gpu_second_trips.py: (operation, shape)
CASES = [(IO, IO_SHAPE), (START, START_SHAPE), (START, IO_SHAPE), (PROLONG, PROLONG_FINE), (RESTRICT, RESTRICT_FINE),
         (ENERGY_REDUCE, ENERGY_REDUCE_SHAPE), (ENERGY_TERMS, ENERGY_TERMS_SHAPE), (ENERGY_REDUCE, ENERGY_TERMS_SHAPE)] + \
        [(ROWS, s) for s in ROW_SHAPES + [SCORE_THREE_ROWS]]


def counts(op, h, w):
    """(items, nblk, takers): the units a member of h x w shares out, its workgroups, and the units a workgroup takes per trip"""
    from chan_vese_amd import capi
    fn = C.CDLL(capi.LIB_PATH).cvh_debug_trip_counts
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    items, nblk, takers = C.c_ulonglong(), C.c_uint(), C.c_uint()
    rc = fn(op, h, w, C.byref(items), C.byref(nblk), C.byref(takers))
    assert rc == 0, (op, h, w, rc)
    return items.value, nblk.value, takers.value


def first_trip(op, h, w):
    """the units taken on the first trip: unit i >= first_trip(...) is somebody's second or later one"""
    _, nblk, takers = counts(op, h, w)
    return nblk * takers


def trips(op, h, w):
    """the trips of the busiest lane, wave or workgroup"""
    items, nblk, takers = counts(op, h, w)
    return max(1, -(-items // (nblk * takers)))
