"""What the adaptive tile schedule computes (csrc/trace.hip's
order_kernel, plan_kernel and the Schedule's launch stages), beyond the bits
of the frame that tests/test_gpu_schedule.py holds: the sort is longest first
over the documented 256 log-scale buckets and halves the record once, the plan
deals a launch's units as its comment says, and inside real launches the cost
record grows by tile index, decays once per launch and drives the next order.

The references are restated here from the comments above the kernels, in
Python integers: bucket() and plan().  rt_schedule_sort runs the two kernels on
chosen data; rt_schedule_read copies a stream's entry out without touching it.
The order within a bucket is arbitrary by design: nothing is asserted on it.
"""
import ctypes as C

import numpy as np
import pytest

SMAX = 64   # policy::kSplitMax: the most units of one tile


# ---- the restatements ---------------------------------------------------------
def bucket(c: int) -> int:
    """A cost's bucket: the cost itself below 8, else five bits of exponent
    (the position e of the leading one, from 3) over the three bits below it."""
    c = int(c)
    if c < 8:
        return c
    e = c.bit_length() - 1
    return ((e - 2) << 3) | ((c >> (e - 3)) & 7)


def buckets(c: np.ndarray) -> np.ndarray:
    """bucket() over a uint32 array (the exponent through frexp: every u32 is
    exact in a double); test_bucket_restatement holds it to bucket()."""
    c = np.asarray(c, np.uint64)
    _, ex = np.frexp(c.astype(np.float64))
    e = np.maximum(ex.astype(np.int64) - 1, 3)
    big = ((e - 2) << 3) | ((c.astype(np.int64) >> (e - 3)) & 7)
    return np.where(c < 8, c.astype(np.int64), big)


def plan(cost_halved, order, U: int, smax: int) -> np.ndarray:
    """The split plan of U units over the tiles in `order` with the record
    `cost_halved`, int32 (U, 2), in exact integers: position p gets
    min(smax, 1 + cost_p (U - n) // total) units (1 + (U - n) // n where the
    total is 0), the units then left over go one each to the first positions
    that are below smax, unit k of a tile's s is (tile, k | s << 8), laid out
    by position, and the rest are (-1, 0)."""
    order = [int(t) for t in order]
    n = len(order)
    cost = [int(cost_halved[t]) for t in order]
    spare, tot = U - n, sum(cost)
    if tot:
        s = [min(smax, 1 + c * spare // tot) for c in cost]
    else:
        s = [min(smax, 1 + spare // n)] * n
    left = max(0, U - sum(s))
    s = [r + 1 if (p < left and r < smax) else r for p, r in enumerate(s)]
    s = np.array(s, np.int64)
    used = int(s.sum())
    assert used <= U
    out = np.empty((U, 2), np.int32)
    out[:used, 0] = np.repeat(np.array(order, np.int64), s)
    k = np.arange(used) - np.repeat(np.cumsum(s) - s, s)
    out[:used, 1] = k | (np.repeat(s, s) << 8)
    out[used:] = (-1, 0)
    return out


def _edges():
    """every 2^k - 1, 2^k, 2^k + 1 within u32"""
    v = sorted({x for k in range(33) for x in (2 ** k - 1, 2 ** k, 2 ** k + 1) if 0 <= x < 2 ** 32})
    return v


def test_bucket_restatement():
    """The restated bucket is monotone non-decreasing and below 256, over all
    c < 2^16 and around every power of two up to 2^32 - 1; the array form is
    the scalar one."""
    small = [bucket(c) for c in range(1 << 16)]
    assert all(a <= b for a, b in zip(small, small[1:]))
    edges = _edges()
    assert edges[-1] == 2 ** 32 - 1
    eb = [bucket(c) for c in edges]
    assert all(a <= b for a, b in zip(eb, eb[1:]))
    assert min(small + eb) == 0 and max(small + eb) == bucket(2 ** 32 - 1) == 239 < 256   # (29 << 3) | 7
    assert bucket(7) == 7 and bucket(8) == 8 and bucket(15) == 15 and bucket(16) == 16 and bucket(2 ** 31) == 232
    assert np.array_equal(buckets(np.arange(1 << 16, dtype=np.uint32)), np.array(small))
    assert np.array_equal(buckets(np.array(edges, np.uint32)), np.array(eb))


# ---- the sort kernel on chosen data --------------------------------------------
def _costs(n: int):
    """The cost sets of the sort test, uint32 (n,) each."""
    rng = np.random.default_rng(1000 + n)
    i = np.arange(n, dtype=np.uint64)
    top = 2 ** 32 - 1
    ramp = (i * top // max(n - 1, 1)).astype(np.uint32)
    edges = np.array(_edges(), np.uint32)
    return {
        "zero": np.zeros(n, np.uint32),
        "equal": np.full(n, 1000, np.uint32),
        "0..7": (i % 8).astype(np.uint32),
        "powers of two and neighbours": np.resize(edges, n),
        "2^32-1": np.full(n, top, np.uint32),
        "ascending": ramp,
        "descending": ramp[::-1].copy(),
        "log-uniform": np.minimum(np.floor(2.0 ** rng.uniform(0.0, 32.0, n)), top).astype(np.uint32),
    }


def _check_sorted(order, cost_in, what):
    n = cost_in.size
    assert np.array_equal(np.sort(order), np.arange(n)), f"{what}: the order is no permutation of 0..{n - 1}"
    b = buckets(cost_in)[order]
    bad = np.nonzero(b[1:] > b[:-1])[0]
    assert bad.size == 0, f"{what}: bucket rises at position {bad[:1]}: {b[bad[:1]]} -> {b[bad[:1] + 1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 7, 255, 1023, 1024, 1025, 4097, 518400])
def test_sort_kernel_orders_longest_first_and_halves_once(gpu_lib, n):
    """order_kernel through rt_schedule_sort (U = 0), the order going up
    filled with -1: a permutation, buckets non-increasing along it, every
    cost halved exactly once.  518,400 is C4's tile count."""
    from rtclj import raytracing as R
    for what, cost in _costs(n).items():
        half, order, _ = R.schedule_sort(cost)
        _check_sorted(order, cost, f"n={n}, {what}")
        assert np.array_equal(half, cost >> 1), f"n={n}, {what}: the costs are not halved once"


# ---- the plan kernel on chosen data ---------------------------------------------
def _plan_cases(n: int):
    """(name, cost, U, smax)"""
    rng = np.random.default_rng(2000 + n)
    rnd = np.floor(2.0 ** rng.uniform(0.0, 24.0, n)).astype(np.uint32)    # durations as launches record them
    wide = np.minimum(np.floor(2.0 ** rng.uniform(0.0, 32.0, n)), 2 ** 32 - 1).astype(np.uint32)
    one = np.zeros(n, np.uint32)
    one[n // 2] = 2 ** 32 - 1
    tiny = (np.arange(n) % 2).astype(np.uint32)                           # 0 and 1: every halved cost is 0
    return [
        ("U = n", rnd, n, 4),
        ("U = n + 1", rnd, n + 1, 4),
        ("U = 3n", rnd, 3 * n, 6),
        ("U = 3n, whole u32 range", wide, 3 * n, 6),
        ("U = n smax", rnd, 4 * n, 4),
        ("U > n smax", rnd, 4 * n + 17, 4),
        ("total 0, U = 3n", np.zeros(n, np.uint32), 3 * n, 6),
        ("total 0 after halving, U = 3n + 1", tiny, 3 * n + 1, 6),
        ("total 0, clamped", np.zeros(n, np.uint32), 9 * n + 5, 4),
        ("smax = 1", rnd, 2 * n, 1),
        ("smax = 64", wide, 40 * n, SMAX),
        ("smax = 64, U = 64n", rnd, SMAX * n, SMAX),
        ("one 2^32-1 among zeros", one, 3 * n, SMAX),
        ("one 2^32-1 among zeros, U = n + 1", one, n + 1, SMAX),
        ("equal costs", np.full(n, 77777, np.uint32), 3 * n + n // 2, 6),
    ]


def _check_plan(units, order, cost_in, U, smax, what):
    """The plan's structure, asserted directly (a failure reads better than a
    mismatch of tables), then the whole table against plan()."""
    n = cost_in.size
    tile, word = units[:, 0].astype(np.int64), units[:, 1].astype(np.int64)
    live = tile >= 0
    used = int(live.sum())
    assert used <= U and np.all(live[:used]) and not np.any(live[used:]), f"{what}: live units are not a prefix"
    assert np.all(word[~live] == 0), f"{what}: an unused unit is not (-1, 0)"
    assert np.all(tile[live] < n), f"{what}: a unit names tile {tile[live].max()} of {n}"
    k, s = word[live] & 0xff, word[live] >> 8
    assert np.all((s >= 1) & (s <= smax)), f"{what}: a tile has {s.max()} units, smax {smax}"
    per = np.bincount(tile[live], minlength=n)
    assert np.all(per >= 1), f"{what}: tile {int(np.argmin(per))} has no unit"
    assert np.array_equal(per[tile[live]], s), f"{what}: a unit's s is not its tile's unit count"
    # each tile's k are 0..s-1 once each: distinct (tile, k) pairs with k < s
    assert np.all(k < s) and np.unique(tile[live] * 256 + k).size == used, f"{what}: a tile's k are not 0..s-1 once each"
    # a tile of a heavier bucket never has fewer units than one of a lighter bucket
    b = buckets(cost_in)
    lo = np.full(256, np.iinfo(np.int64).max)
    hi = np.zeros(256, np.int64)
    np.minimum.at(lo, b, per)
    np.maximum.at(hi, b, per)
    fewest_above = np.minimum.accumulate(lo[::-1])[::-1]   # over buckets >= b
    for bb in np.unique(b)[:-1]:
        assert hi[bb] <= fewest_above[bb + 1], f"{what}: bucket {bb} has a tile of {hi[bb]} units, a heavier one fewer"
    want = plan(cost_in >> 1, order, U, smax)
    diff = np.nonzero(np.any(units != want, axis=1))[0]
    assert diff.size == 0, f"{what}: unit {diff[0]} is {units[diff[0]]}, the plan has {want[diff[0]]} ({diff.size} differ)"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1025, 4097])
def test_plan_kernel_deals_units_by_cost(gpu_lib, n):
    """plan_kernel behind order_kernel (rt_schedule_sort, U > 0), on the
    device's own order of the same call: the units, going up filled with -1,
    equal the restated plan bit for bit.  n = 1, 1023, 1025, 4097: a thread
    owns no, one or several positions."""
    from rtclj import raytracing as R
    for what, cost, U, smax in _plan_cases(n):
        half, order, units = R.schedule_sort(cost, units=U, smax=smax)
        what = f"n={n}, {what}"
        _check_sorted(order, cost, what)
        assert np.array_equal(half, cost >> 1), what
        _check_plan(units, order, cost, U, smax, what)


@pytest.mark.gpu
def test_plan_kernel_large_products(gpu_lib):
    """cost x spare far beyond 2^32 and beyond a double's 53 bits: three tiles
    of 2^32 - 1, 2^32 - 2 and 3 with U = 2^24 + 3 (product 2^55), smax 64 and
    smax 1; every unit past the clamps is (-1, 0).  (A halved cost is below
    2^31 and the spare units below 2^31, so the product stays below 2^62: U
    is as large as a quick test's 128 MB table allows.)"""
    from rtclj import raytracing as R
    cost = np.array([3, 2 ** 32 - 1, 2 ** 32 - 2], np.uint32)
    U = 2 ** 24 + 3
    for smax in (SMAX, 1):
        _, order, units = R.schedule_sort(cost, units=U, smax=smax)
        _check_sorted(order, cost, "large products")
        _check_plan(units, order, cost, U, smax, f"large products, smax {smax}")
    # shares the clamp does not touch, of the largest costs: 60 spare units over 2^31 - 1, 1, 2^31 - 1, 2^30
    cost = np.array([2 ** 32 - 1, 2, 2 ** 32 - 1, 2 ** 31], np.uint32)
    _, order, units = R.schedule_sort(cost, units=4 + 60, smax=SMAX)
    _check_plan(units, order, cost, 64, SMAX, "large costs, unclamped")


# ---- the schedule inside real launches -------------------------------------------
KNOBS = ("RTCLJ_SPLIT", "RTCLJ_SPLIT_PLAN", "RTCLJ_SORT_EAGER", "RTCLJ_FIRST_ORDER", "RTCLJ_EXPORT")
SHAPES = [(96, 54), (333, 187)]   # the second: ragged tiles at both edges
SPP = 6


class Run:
    """cover(11) uploaded for one test, on a stream of its own."""

    def __init__(self):
        import torch
        from rtclj import scenes
        from rtclj._lib import check, lib
        self.torch, self.lib = torch, lib
        self.sc = scenes.cover(11)
        self.ds = C.c_void_p()
        check(lib.rt_scene_upload(0, C.byref(self.sc.c), C.byref(self.ds)))
        self.stream = torch.cuda.Stream()

    def close(self):
        self.torch.cuda.synchronize()
        self.lib.rt_scene_free(self.ds)

    def params(self, w, h, spp=SPP, max_depth=50):
        from rtclj._lib import rt_params
        return rt_params(width=w, height=h, row_begin=0, row_end=h, spp=spp, max_depth=max_depth, seed=1)

    def launch(self, w, h, spp=SPP, stream=None):
        """rt_launch into a NaN-filled buffer on the stream; the frame."""
        from rtclj import scenes
        s = stream or self.stream
        cam, p = scenes.cover_camera(w, h), self.params(w, h, spp)
        with self.torch.cuda.stream(s):
            out = self.torch.full((h * w * 3,), float("nan"), dtype=self.torch.float32, device="cuda")
        s.synchronize()
        rc = self.lib.rt_launch(self.ds, C.byref(cam), C.byref(p), C.c_void_p(out.data_ptr()), None,
                                C.c_void_p(s.cuda_stream))
        assert rc == 0, self.lib.rt_last_error()
        s.synchronize()
        return out.cpu().numpy().reshape(h, w, 3)

    def read(self, stream=None, arrays=True):
        from rtclj import raytracing as R
        return R.schedule_read(self.ds, (stream or self.stream).cuda_stream, arrays=arrays)

    def want(self, w, h, spp=SPP):
        from rtclj import raytracing as R
        from rtclj import scenes
        return R.render(self.sc, scenes.cover_camera(w, h), w, h, spp=spp, max_depth=50)


@pytest.fixture
def run(gpu_lib, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    r = Run()
    yield r
    r.close()


def _tiles(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


def _first_order(n):
    return np.arange(n - 1, -1, -1, dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("knobs", [
    dict(),                                          # the launch's own choice of a split
    dict(RTCLJ_SPLIT="1"),                           # whole tiles: one workgroup's life per tile (and tile sharing)
    dict(RTCLJ_SPLIT="4"),                           # every tile four units: the gains come from split units
    dict(RTCLJ_SPLIT="4", RTCLJ_SPLIT_PLAN="1"),     # ... dealt by the plan from launch 2 on
], ids=lambda k: "-".join(f"{n[6:].lower()}{v}" for n, v in k.items()) or "default")
def test_record_grows_decays_and_orders_the_next_launch(run, monkeypatch, knobs, shape):
    """Three launches of one shape, the entry read after each.  Launch 1: the
    bottom-up first order, every tile's cost positive, the sort pending.
    Launch k > 1: its order O_k is a permutation whose buckets of the
    record C_(k-1) do not rise (the sort ran on the previous record), and
    C_k[i] > C_(k-1)[i] >> 1 for every tile i (the record was halved once and
    this launch added to every tile, by tile index).  With the plan on, the
    units read after launch k are plan(C_(k-1) >> 1, O_k) for 4n units, and
    the frames stay rt_render's."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    w, h = shape
    n = _tiles(w, h)
    planned = "RTCLJ_SPLIT_PLAN" in knobs
    want = run.want(w, h) if planned else None
    prev = None
    for launch in (1, 2, 3):
        frame = run.launch(w, h)
        info, cost, order, units = run.read()
        assert info["exists"] == 1 and info["n_tiles"] == n and info["has_record"] == 1, info
        assert info["ready"] == 0 and info["sort_pending"] == 1, (launch, info)
        if planned:
            assert np.array_equal(frame, want), launch
            assert info["sort_plan"] == 4 * n and info["plan_units"] == (4 * n if launch > 1 else -1), (launch, info)
        else:
            assert info["plan_units"] == -1 and units.size == 0, (launch, info)
        if launch == 1:
            assert np.array_equal(order, _first_order(n)), "launch 1 is not in the bottom-up first order"
            assert cost.min() > 0, f"launch 1 left tile {int(cost.argmin())} without a cost"
            print(f"{w}x{h} {knobs}: launch 1 costs {cost.min()} .. {cost.max()} ticks (100 MHz)")
        else:
            _check_sorted(order, prev, f"launch {launch}: the order against the record before it")
            gain = cost.astype(np.int64) - (prev >> 1).astype(np.int64)
            print(f"{w}x{h} {knobs}: launch {launch} smallest per-tile gain {gain.min()} ticks, largest {gain.max()}")
            assert gain.min() > 0, f"launch {launch}: tile {int(gain.argmin())} gained {gain.min()} over half its record"
            if planned:
                assert np.array_equal(units, plan(prev >> 1, order, 4 * n, min(SPP, SMAX))), launch
        prev = cost


def _log_distance(a, b):
    return float(np.abs(np.log(a.astype(np.float64)) - np.log(b.astype(np.float64))).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["1", "4"])
def test_cost_is_recorded_by_tile_index_not_order_position(run, monkeypatch, split):
    """A tile's work does not depend on when it is dispatched, so its cost is
    the same, up to noise, under any order.  The yardstick R is the record of a
    first launch in row-major order (RTCLJ_FIRST_ORDER=0: position = tile, no
    order to confuse them) on a second stream.  Against it, by tile index:
    launch 1 in the bottom-up order gives C_1, which must be nearer R than R
    mirrored (what adding at the order position n - 1 - i would record: the
    sky is at the top of this frame, the ground at the bottom); launch 2 in
    the sorted order O_2 gains G_2, which must be nearer R than R[O_2] (what
    adding at the position would record).  Distances are sums of |log a -
    log b| over the tiles; no threshold is involved."""
    monkeypatch.setenv("RTCLJ_SPLIT", split)
    w, h, spp = 160, 90, 16
    other = run.torch.cuda.Stream()
    monkeypatch.setenv("RTCLJ_FIRST_ORDER", "0")
    run.launch(w, h, spp, stream=other)
    ref = run.read(stream=other)[1]
    monkeypatch.delenv("RTCLJ_FIRST_ORDER")
    run.launch(w, h, spp)
    _, c1, o1, _ = run.read()
    assert np.array_equal(o1, _first_order(c1.size)) and ref.min() > 0 and c1.min() > 0
    d_tile, d_pos = _log_distance(c1, ref), _log_distance(c1, ref[::-1])
    print(f"split {split}: launch 1 against the row-major record: by tile {d_tile:.1f}, by position {d_pos:.1f}")
    assert d_tile < d_pos, "launch 1's costs follow the order position, not the tile"
    run.launch(w, h, spp)
    _, c2, o2, _ = run.read()
    gain = c2.astype(np.int64) - (c1 >> 1).astype(np.int64)
    assert gain.min() > 0
    d_tile, d_pos = _log_distance(gain, ref), _log_distance(gain, ref[o2])
    print(f"split {split}: launch 2's gains against the row-major record: by tile {d_tile:.1f}, by position {d_pos:.1f}")
    assert d_tile < d_pos, "launch 2's gains follow the order position, not the tile"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_eager_sort_shows_the_sorted_halved_record(run, monkeypatch, shape):
    """RTCLJ_SORT_EAGER=1 sorts right behind each launch, so the read after
    launch k already shows H_k = C_k >> 1, the order O of C_k, ready == 1 and
    no sort pending.  The relations shift accordingly.  bucket(c >> 1) is a
    non-decreasing function of bucket(c) (bucket(c) - 8 from 16 on, c >> 1
    below), so the buckets of H_k do not rise along O either.  And C_k =
    H_(k-1) + gain with gain >= 1 gives 2 H_k + 1 >= C_k > H_(k-1), that is
    2 H_k >= H_(k-1) for every tile; H_1 > 0 as a workgroup lives longer than
    two ticks."""
    monkeypatch.setenv("RTCLJ_SORT_EAGER", "1")
    w, h = shape
    n = _tiles(w, h)
    prev = None
    for launch in (1, 2, 3):
        run.launch(w, h)
        info, half, order, _ = run.read()
        assert info["exists"] == 1 and info["n_tiles"] == n, info
        assert info["ready"] == 1 and info["sort_pending"] == 0, (launch, info)
        _check_sorted(order, half, f"eager, launch {launch}")
        assert half.min() > 0, launch
        if prev is not None:
            low = 2 * half.astype(np.int64) - prev.astype(np.int64)
            print(f"{w}x{h} eager: launch {launch} smallest per-tile gain {low.min()} or {low.min() + 1} ticks")
            assert low.min() >= 0, f"launch {launch}: tile {int(low.argmin())}"
        prev = half


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plain_order_leaves_the_record_alone(run, shape):
    """rt_set_schedule(1): a launch neither reads nor writes the record."""
    w, h = shape
    want = run.want(w, h)
    for _ in range(2):
        run.launch(w, h)
    before = run.read()
    old = run.lib.rt_set_schedule(1)
    try:
        frame = run.launch(w, h)
    finally:
        run.lib.rt_set_schedule(old)
    after = run.read()
    assert np.array_equal(frame, want)
    assert before[0] == after[0], (before[0], after[0])
    for a, b in zip(before[1:], after[1:]):
        assert a.tobytes() == b.tobytes()
    # and the next scheduled launch goes on from that record
    run.launch(w, h)
    info, cost, order, _ = run.read()
    _check_sorted(order, before[1], "the launch after plain order")
    assert np.all(cost.astype(np.int64) > (before[1] >> 1).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_another_shape_starts_the_record_again(run, shape):
    """A launch of another shape in between re-keys the entry (ready back to
    0, its own tile count), and the next launch of the first shape is a first
    order again with a record of its own."""
    w, h = shape
    n = _tiles(w, h)
    for _ in range(2):
        run.launch(w, h)
    assert run.read(arrays=False)[0]["n_tiles"] == n
    run.launch(64, 40)
    info, cost, order, _ = run.read()
    assert info["n_tiles"] == _tiles(64, 40) and info["ready"] == 0 and info["sort_pending"] == 1, info
    assert np.array_equal(order, _first_order(_tiles(64, 40))) and cost.min() > 0
    run.launch(w, h)
    info, cost, order, _ = run.read()
    assert info["n_tiles"] == n and info["ready"] == 0 and info["sort_pending"] == 1, info
    assert np.array_equal(order, _first_order(n)), "not a first order after another shape's launch"
    assert cost.min() > 0
    first = cost
    run.launch(w, h)
    info, cost, order, _ = run.read()
    _check_sorted(order, first, "the second launch after the re-key")
    assert np.all(cost.astype(np.int64) > (first >> 1).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_other_passes_leave_the_record_alone(run, shape):
    """rt_launch_feat, rt_adapt_step (rt_launch_accum's pass over the active
    tiles) and rt_launch_ids on the same scene and stream: the entry reads
    back unchanged byte for byte, as include/rt.h says of each.  (A plain
    rt_launch_accum pass uses and feeds the record as rt_launch does; the last
    lines hold it to that.)"""
    from rtclj import scenes
    from rtclj._lib import check, rt_adapt_opts
    lib, torch = run.lib, run.torch
    w, h = shape
    cam, st = scenes.cover_camera(w, h), C.c_void_p(run.stream.cuda_stream)
    for _ in range(2):
        run.launch(w, h)
    before = run.read()
    assert before[0]["sort_pending"] == 1
    ft, ad, acc = C.c_void_p(), C.c_void_p(), C.c_void_p()
    p = run.params(w, h, spp=2)
    try:
        pf = run.params(w, h, spp=2, max_depth=1)
        check(lib.rt_feat_create(run.ds, C.byref(pf), C.byref(ft)))
        check(lib.rt_launch_feat(run.ds, C.byref(cam), C.byref(pf), ft, None, st))
        opts = rt_adapt_opts(step_spp=2, min_spp=4, max_spp=8, tol_q16=2048)
        check(lib.rt_adapt_create(run.ds, C.byref(p), C.byref(opts), C.byref(ad)))
        traced = [check(lib.rt_adapt_step(run.ds, C.byref(cam), C.byref(p), ad, None, st)) for _ in range(3)]
        assert traced[0] == _tiles(w, h) and traced[1] > 0, traced
        with torch.cuda.stream(run.stream):
            ids = torch.full((h * w,), -7, dtype=torch.int32, device="cuda")
        run.stream.synchronize()
        check(lib.rt_launch_ids(run.ds, C.byref(cam), w, h, 0, C.c_void_p(ids.data_ptr()), st))
        run.stream.synchronize()
        assert int(ids.min()) >= -1                       # (the pass ran)
        after = run.read()
        assert before[0] == after[0], (before[0], after[0])
        for a, b in zip(before[1:], after[1:]):
            assert a.tobytes() == b.tobytes()
        check(lib.rt_accum_create(run.ds, C.byref(p), C.byref(acc)))
        check(lib.rt_launch_accum(run.ds, C.byref(cam), C.byref(p), acc, None, st))
        info, cost, order, _ = run.read()
        assert info["sort_pending"] == 1
        _check_sorted(order, before[1], "rt_launch_accum's pass")
        assert np.all(cost.astype(np.int64) > (before[1] >> 1).astype(np.int64))
    finally:
        run.stream.synchronize()
        if acc:
            lib.rt_accum_free(acc)
        if ad:
            lib.rt_adapt_free(ad)
        if ft:
            lib.rt_feat_free(ft)


@pytest.mark.gpu
def test_schedule_read_caps_and_absent_entries(run):
    """rt_schedule_read: info only with NULL buffers; a cap below the tile or
    unit count is RT_E_ARG and writes nothing; a stream that never launched
    owns no entry; reading twice gives the same bytes (nothing is changed)."""
    from rtclj._lib import i32ptr, rt_schedule_info, u32ptr
    lib = run.lib
    w, h = 96, 54
    n = _tiles(w, h)
    other = run.torch.cuda.Stream()
    info = run.read(stream=other, arrays=False)[0]
    assert info["exists"] == 0 and info["n_tiles"] == 0 and info["plan_units"] == -1 and info["max_streams"] == 16, info
    run.launch(w, h)
    run.launch(w, h)
    a, b = run.read(), run.read()
    assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    assert run.read(stream=other, arrays=False)[0]["exists"] == 0
    st = C.c_void_p(run.stream.cuda_stream)
    inf = rt_schedule_info(n_tiles=-9)
    cost, order = np.full(n, 0xdeadbeef, np.uint32), np.full(n, -9, np.int32)
    assert lib.rt_schedule_read(run.ds, st, C.byref(inf), u32ptr(cost), i32ptr(order), None, n - 1, 0) == -1
    assert b"cap_tiles" in lib.rt_last_error()
    assert inf.n_tiles == -9 and np.all(cost == 0xdeadbeef) and np.all(order == -9)
    assert lib.rt_schedule_read(run.ds, st, C.byref(inf), u32ptr(cost), None, None, n, 0) == 0
    assert inf.n_tiles == n and np.array_equal(cost, a[1]) and np.all(order == -9)


@pytest.mark.gpu
def test_recorded_cost_means_work(run):
    """The record measures work: cover(11) at 160 x 90, 32 spp, after three
    launches; tiles whose every pixel centre sees the sky (rt_launch_ids: -1
    throughout) against the rest.  The ratio of the median recorded costs,
    non-sky over sky, is printed (DESIGN.md §3.1 carries the MI355X's figure,
    9.2: 24 sky tiles at 22,818 ticks, 216 others at 210,306) and held above
    1 -- a bound that owes nothing to the figure: work is more than none."""
    from rtclj import scenes
    from rtclj._lib import check
    w, h, spp = 160, 90, 32
    gx, gy = (w + 7) // 8, (h + 7) // 8
    for _ in range(3):
        run.launch(w, h, spp)
    info, cost, _, _ = run.read()
    assert info["n_tiles"] == gx * gy
    cam = scenes.cover_camera(w, h)
    with run.torch.cuda.stream(run.stream):
        ids = run.torch.full((h * w,), -7, dtype=run.torch.int32, device="cuda")
    run.stream.synchronize()
    check(run.lib.rt_launch_ids(run.ds, C.byref(cam), w, h, 0, C.c_void_p(ids.data_ptr()),
                                C.c_void_p(run.stream.cuda_stream)))
    run.stream.synchronize()
    hit = np.zeros((gy * 8, gx * 8), bool)
    hit[:h, :w] = ids.cpu().numpy().reshape(h, w) >= 0
    sky = ~hit.reshape(gy, 8, gx, 8).any(axis=(1, 3)).reshape(-1)
    assert 0 < sky.sum() < sky.size, f"{int(sky.sum())} of {sky.size} tiles are all sky"
    m_sky, m_rest = float(np.median(cost[sky])), float(np.median(cost[~sky]))
    print(f"recorded cost, {w}x{h} {spp} spp: {int(sky.sum())} sky tiles median {m_sky:.0f} ticks, "
          f"{int((~sky).sum())} others median {m_rest:.0f}: ratio {m_rest / m_sky:.2f}")
    assert m_sky > 0
    assert m_rest / m_sky > 1, "tiles with bodies record no more cost than tiles of sky"   # (the MI355X measures 9.2)
