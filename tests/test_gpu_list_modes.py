"""Every launch mode of the path kernel over frames whose tiles list bodies
(DESIGN.md §3.1, §3.2).  The mode tests that predate the camera prelude's list
render frames so small that most of their tiles list more than 14 bodies and
take the walk; the list's own tests run at sample counts at which no tile is
shared.  Here each mode -- tile sharing and helpers, sample splits and the
cost-balanced plan, drain compaction, wrap-counting sums, accumulating passes,
the adaptive step, the budget's passes and its fused unit table, a refit
between frames, frames in flight, path export -- runs over tests/body_list_scenes.py's
"40x24" (15 whole tiles listing 0 .. 14 bodies) and "44x27m" (24 tiles, partial
ones at the right and the bottom; 15 list 1 .. 14 bodies, 8 overflow and take
the walk; tests/test_list_mode_scenes.py holds those counts on the host).

Every case renders under variant 30 (the walk alone), variant 22 (the list) and
the default choice, which must resolve to 22, and compares frame, segments and
samples bit for bit among the three and with the oracle's fp32 mirror
(MODE_MIRROR32 | DIRECT; for the integer sums of items 5 to 7, the mirror's
one-sample frames, which are exact integers).  Each case also asserts that its
mode engaged, by what the library lets a caller read back; where it lets
nothing be read (a compaction post, a helperless shared tile) the case states
the launch's property that puts it on that path.  The knobs are read at every
launch.  Depth 6, the loop-free samplers; one RT_FLAG_REJECTION_SAMPLERS and
one RT_FLAG_REALM case per mode.

Path export (RTCLJ_EXPORT) is a mode of the list's kernel alone: only variant
22 has a sweep (trace.hip, variant_sweep), and the launch that writes the
records out is variant 22 itself, prelude, gate and list; the sweep that runs
them has no prelude.  Left out: 8 x 4 pools (RTCLJ_TH4: variant 28 is not
instantiated with the prelude).
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import body_list_scenes as B  # noqa: E402
from list_mode_support import (DEFAULT, DEPTH, LIST, WALK, each_variant, launch, mirror, mirror_ints, per_pixel,  # noqa: E402
                               resolved, same, shard_bands, uploaded)
from test_gpu_accum import Acc  # noqa: E402
from test_gpu_adapt import OPTS, Ad, simulate  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 3
SHARING = dict(RTCLJ_SPLIT="1", RTCLJ_SHARE_RECORDED="1")
FLAGS = ("direct", "rejection", "realm")


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu_lib):
    import torch
    e = Env()
    e.torch, e.lib = torch, gpu_lib.lib
    e.frames = {name: B.frame(name) for name in B.MODE_FRAMES}
    e.counts = {name: np.array([len(b) for b, _ in B.tile_lists(sc, cam, B.params(w, h))])
                for name, (sc, cam, w, h) in e.frames.items()}
    e.stream = torch.cuda.Stream()
    return e


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    """Every case starts from the library's defaults."""
    for k in ("RTCLJ_SPLIT", "RTCLJ_SHARE_RECORDED", "RTCLJ_STEAL_MIN", "RTCLJ_BATCH_MAX", "RTCLJ_THIEVES", "RTCLJ_COMPACT",
              "RTCLJ_SPLIT_PLAN", "RTCLJ_STEAL", "RTCLJ_EXPORT", "RTCLJ_EXPORT_LIM", "RTCLJ_TH4"):
        monkeypatch.delenv(k, raising=False)


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))


def _flag(which):
    from rtclj import _lib
    return {"direct": 0, "rejection": _lib.RT_FLAG_REJECTION_SAMPLERS, "realm": _lib.RT_FLAG_REALM}[which]


def _steals(env, ds):
    st = (C.c_uint64 * 2)()
    assert env.lib.rt_steal_stats(ds, C.c_void_p(env.stream.cuda_stream), st) == 0
    return int(st[0]), int(st[1])


# ---- 1. tile sharing and helpers --------------------------------------------------------------
def _shared_frames(env, spps, flags=0, shard=None, lens=0.0):
    """Both frames at each spp, twice on one stream of a fresh upload (plain
    order, then the recorded one), under the three variants, each launch
    against the mirror -> {(name, spp): {variant: [(steals, samples)] * 2}}."""
    out = {}
    for name in B.MODE_FRAMES:
        sc, cam, w, h = env.frames[name]
        if lens:
            cam = B.camera(w, h, lens)
        for spp in spps:
            kw = dict(row_tile=8, tile_first=shard[0], tile_step=shard[1]) if shard else {}
            p = B.params(w, h, spp=spp, flags=flags, **kw)
            p.seed = SEED
            want = mirror(f"{name} lens {lens}" if lens else name, sc, cam, w, h, spp, SEED, flags,
                          bands=shard_bands(h, 8, *shard) if shard else None)

            def run(v):
                stats = []
                with uploaded(sc) as ds:
                    resolved(ds, p, v)
                    for k in range(2):
                        same(launch(ds, cam, p, env.stream), want, f"{name} {spp} spp variant {v} launch {k}")
                        stats.append(_steals(env, ds))
                return stats
            out[(name, spp)] = each_variant(run)
    return out


@pytest.mark.parametrize("knobs", [dict(RTCLJ_STEAL_MIN=1), dict(RTCLJ_STEAL_MIN=1, RTCLJ_BATCH_MAX=65536),
                                   dict(RTCLJ_THIEVES=0), dict(RTCLJ_THIEVES=1), dict(RTCLJ_THIEVES=16)],
                         ids=lambda k: "-".join(f"{n[6:].lower()}{v}" for n, v in k.items()))
def test_shared_tiles(env, monkeypatch, knobs):
    """Whole tiles (RTCLJ_SPLIT=1), shared in the recorded order too.  At 9 spp
    a whole tile's pool is 576, the smallest the kernel shares (pool > 512),
    and 44x27m's partial tiles (288 and 216 samples) are not shared; at 40 spp
    every tile is.  Engaged: with helpers joining any tile that has an
    unclaimed sample (STEAL_MIN=1), at 40 spp, rt_steal_stats reports steals
    and 0 < helpers' samples < all samples, under each variant, in each frame
    and in each of its two launches; with no helper
    workgroups (THIEVES=0: the owners alone claim from the shared word) none."""
    _set(monkeypatch, {**SHARING, **knobs})
    assert 64 * 9 > 512 >= 64 * 8 and 4 * 8 * 9 <= 512 and 8 * 3 * 9 <= 512
    got = _shared_frames(env, (9, 40))
    for v in (WALK, LIST, DEFAULT):
        at40 = [st for (name, spp), by in got.items() if spp == 40 for st in by[v]]
        steals, helped = sum(s for s, _ in at40), sum(n for _, n in at40)
        total = 2 * 40 * sum(w * h for _, _, w, h in env.frames.values())
        print(knobs, v, steals, helped, total)
        if "RTCLJ_STEAL_MIN" in knobs:
            assert steals > 0 and 0 < helped < total, (v, steals, helped, total)
            for name in B.MODE_FRAMES:   # ... in each frame, in plain order and in the recorded one
                _, _, w, h = env.frames[name]
                for k, (s, n) in enumerate(got[(name, 40)][v]):
                    print(name, v, k, s, n)
                    assert s > 0 and 0 < n < 40 * w * h, (name, v, k, s, n)
        if knobs.get("RTCLJ_THIEVES") == 0:
            assert all(st == (0, 0) for by in got.values() for st in by[v]), v


def test_shared_tiles_of_an_interleaved_shard(env, monkeypatch):
    """The odd 8-row bands (row_tile 8, tile_first 1, tile_step 2), helpers joining any tile."""
    _set(monkeypatch, {**SHARING, "RTCLJ_STEAL_MIN": 1})
    got = _shared_frames(env, (9, 40), shard=(1, 2))
    assert sum(s for by in got.values() for s, _ in by[LIST]) > 0


def test_shared_tiles_under_a_lens(env, monkeypatch):
    """B.camera(w, h, 0.6): wider lists (a tile's rays start anywhere on the
    disk) and the disk sampler's draws in the trips; 44x27m keeps tiles on both
    sides of the limit."""
    _set(monkeypatch, {**SHARING, "RTCLJ_STEAL_MIN": 1})
    sc, _, w, h = env.frames["44x27m"]
    counts = [len(b) for b, _ in B.tile_lists(sc, B.camera(w, h, 0.6), B.params(w, h))]
    assert sum(1 for c in counts if 1 <= c <= 14) >= 8 and sum(1 for c in counts if c > 14) >= 8, counts
    got = _shared_frames(env, (9, 40), lens=0.6)
    assert sum(s for by in got.values() for s, _ in by[LIST]) > 0


@pytest.mark.parametrize("which", FLAGS[1:])
def test_shared_tiles_flags(env, monkeypatch, which):
    _set(monkeypatch, {**SHARING, "RTCLJ_STEAL_MIN": 1})
    got = _shared_frames(env, (9, 40), flags=_flag(which))
    assert sum(s for by in got.values() for s, _ in by[LIST]) > 0


# ---- 2. sample splits -------------------------------------------------------------------------
def _split_frames(env, monkeypatch, split, spps, flags=0):
    """Five launches on one stream of a fresh upload: plain order, recorded
    order, then with RTCLJ_SPLIT_PLAN=1 one that records a plan and one that
    runs its cost-balanced units, then the plan off again.  Engaged: a wholly
    split launch asks the record's sort for a plan of its unit count
    (rt_schedule_read's sort_plan, then plan_units once the sort has run), and
    that count is tiles x min(split, spp, 64): every tile ran as that many
    units, all but the first from a sample k0 != 0."""
    from rtclj import raytracing as R
    for name in B.MODE_FRAMES:
        sc, cam, w, h = env.frames[name]
        n_tiles = len(env.counts[name])
        for spp in spps:
            p = B.params(w, h, spp=spp, flags=flags)
            p.seed = SEED
            want = mirror(name, sc, cam, w, h, spp, SEED, flags)
            units = n_tiles * min(split or 64, spp, 64)
            assert units > n_tiles

            def run(v):
                def go(k):
                    same(launch(ds, cam, p, env.stream), want, f"{name} {spp} spp split {split} variant {v} launch {k}")
                    return R.schedule_read(ds, env.stream.cuda_stream, arrays=False)[0]
                monkeypatch.delenv("RTCLJ_SPLIT_PLAN", raising=False)
                with uploaded(sc) as ds:
                    resolved(ds, p, v)
                    infos = [go(0), go(1)]
                    monkeypatch.setenv("RTCLJ_SPLIT_PLAN", "1")
                    infos += [go(2), go(3)]
                    monkeypatch.setenv("RTCLJ_SPLIT_PLAN", "0")
                    infos.append(go(4))
                assert infos[1]["sort_plan"] == -1 and infos[2]["sort_plan"] == units, (v, infos)
                assert infos[3]["plan_units"] == units and infos[3]["n_tiles"] == n_tiles, (v, infos)
            each_variant(run)


@pytest.mark.parametrize("split", [None, 2, 3, 5, 64])
def test_sample_splits(env, monkeypatch, split):
    """None: rt_launch's own choice, which splits frames of so few tiles
    (min(spp, 64) units a tile).  64 splits of 7 spp: seven units of one sample."""
    if split is not None:
        monkeypatch.setenv("RTCLJ_SPLIT", str(split))
    _split_frames(env, monkeypatch, split, (7, 40))


@pytest.mark.parametrize("which", FLAGS[1:])
def test_sample_splits_flags(env, monkeypatch, which):
    monkeypatch.setenv("RTCLJ_SPLIT", "3")
    _split_frames(env, monkeypatch, 3, (7, 40), flags=_flag(which))


# ---- 3. drain compaction ----------------------------------------------------------------------
def _drained_frames(env, spps, flags=0):
    for name in B.MODE_FRAMES:
        sc, cam, w, h = env.frames[name]
        for spp in spps:
            p = B.params(w, h, spp=spp, flags=flags)
            p.seed = SEED
            want = mirror(name, sc, cam, w, h, spp, SEED, flags)

            def run(v):
                with uploaded(sc) as ds:
                    resolved(ds, p, v)
                    for k in range(2):
                        same(launch(ds, cam, p, env.stream), want, f"{name} {spp} spp variant {v} launch {k}")
            each_variant(run)


@pytest.mark.parametrize("knobs", [dict(RTCLJ_COMPACT=64, RTCLJ_SPLIT=1), dict(RTCLJ_COMPACT=16, RTCLJ_SPLIT=1),
                                   dict(RTCLJ_COMPACT=1, RTCLJ_SPLIT=1), dict(RTCLJ_COMPACT=0, RTCLJ_SPLIT=1),
                                   dict(RTCLJ_COMPACT=16, RTCLJ_STEAL_MIN=1, **SHARING), dict(RTCLJ_COMPACT=16)],
                         ids=lambda k: "-".join(f"{n[6:].lower()}{v}" for n, v in k.items()))
def test_drain_compaction(env, monkeypatch, knobs):
    """Thresholds 64 (clamped to what the stack slice holds), 16, 1 and 0 (off)
    on whole tiles; 16 with helpers joining any tile; 16 on rt_launch's own
    split units.  At 3 spp a whole tile's pool is 192 samples, fewer than the
    workgroup's 256 lanes: the batches are spent at the start, so the gate
    passes every trip and the drain check runs from the first iteration.  No
    post is observed: neither build counts one (the statistics build's drain
    checks, which test_the_lists_were_used reads, run with compaction off
    too), so what is asserted for this mode is the launch's property above and
    the bits at every threshold."""
    _set(monkeypatch, knobs)
    assert 64 * 3 < 256
    _drained_frames(env, (3, 24, 40))


@pytest.mark.parametrize("which", FLAGS[1:])
def test_drain_compaction_flags(env, monkeypatch, which):
    _set(monkeypatch, dict(RTCLJ_COMPACT=16, RTCLJ_SPLIT=1))
    _drained_frames(env, (3, 24), flags=_flag(which))


# ---- 4. wrap-counting sums --------------------------------------------------------------------
@pytest.mark.parametrize("which", FLAGS)
@pytest.mark.parametrize("knobs", [{}, dict(RTCLJ_STEAL_MIN=1, **SHARING)], ids=["default", "shared"])
def test_sums_count_their_wraps(env, monkeypatch, knobs, which):
    """300 spp on 40x24: above 255 spp the compact image's u32 sums count their
    wraps, in rt_launch's own split units and in whole tiles that helpers
    join.  Engaged: a channel whose mean is at least 256 / 300 summed to 2^32
    or more; the mirror has such pixels (the sky) in tiles with a list."""
    _set(monkeypatch, knobs)
    flags = _flag(which)
    sc, cam, w, h = env.frames["40x24"]
    spp = 300
    p = B.params(w, h, spp=spp, flags=flags)
    p.seed = SEED
    want = mirror("40x24", sc, cam, w, h, spp, SEED, flags)
    wrapped = (want[0].astype(np.float64) * spp >= 256.0).any(axis=-1)
    listed = per_pixel((env.counts["40x24"] >= 1).reshape(3, 5), h, w)
    assert (wrapped & listed).sum() > 64

    def run(v):
        with uploaded(sc) as ds:
            resolved(ds, p, v)
            stats = []
            for k in range(2):
                same(launch(ds, cam, p, env.stream), want, f"300 spp variant {v} launch {k}")
                stats.append(_steals(env, ds))
        return stats
    got = each_variant(run)
    if knobs:
        assert all(sum(s for s, _ in got[v]) > 0 for v in got), got


# ---- 5. accumulating passes -------------------------------------------------------------------
def _accumulated(env, name, sizes, begin, flags=0):
    """rt_launch_accum in passes of `sizes` from sample `begin`: the resolved
    frame and the counters equal the mirror's frame of all the samples, every
    pass alone equals the mirror from its own sample_begin, and the integer
    sums are the same under the three variants.  Engaged: rt_accum_samples, and
    every pass but the first starts at a sample_begin other than the frame's."""
    from rtclj._lib import rt_params
    sc, cam, w, h = env.frames[name]
    total = sum(sizes)
    p = B.params(w, h, spp=total, flags=flags, sample_begin=begin)
    p.seed = SEED
    want = mirror(name, sc, cam, w, h, total, SEED, flags, begin=begin)

    def run(v):
        with uploaded(sc) as ds:
            resolved(ds, p, v)
            acc = Acc(env, p, ds=ds)
            try:
                acc.passes(cam, p, sizes)
                assert acc.samples == total
                same((acc.frame(flags), tuple(acc.counters())), want, f"{name} passes {sizes} from {begin} variant {v}")
                sums = acc.read()
            finally:
                acc.free()
            q = rt_params.from_buffer_copy(p)
            for n in sizes[:2]:
                q.spp = n
                one = Acc(env, q, ds=ds)
                try:
                    one.add(cam, q)
                    same((one.frame(flags), tuple(one.counters())),
                         mirror(name, sc, cam, w, h, n, SEED, flags, begin=q.sample_begin),
                         f"{name} pass of {n} from {q.sample_begin} variant {v}")
                finally:
                    one.free()
                q.sample_begin += n
        return sums
    got = each_variant(run)
    assert got[WALK].any() and np.array_equal(got[WALK], got[LIST]) and np.array_equal(got[LIST], got[DEFAULT])


@pytest.mark.parametrize("sizes,begin", [((3, 5), 0), ((5, 3), 0), ((1,) * 8, 0), ((3, 5), 11), ((3, 5), -4)],
                         ids=["3+5", "5+3", "1x8", "3+5from11", "3+5over2^32"])
@pytest.mark.parametrize("name", B.MODE_FRAMES)
def test_accumulating_passes(env, name, sizes, begin):
    """sample_begin -4 carries the bits of 2^32 - 4 (the kernel keys sample k by
    uint32(sample_begin + k)): the first pass ends at 2^32 - 2, the second runs
    from 2^32 - 1 over the wrap to sample 3."""
    _accumulated(env, name, sizes, begin)


@pytest.mark.parametrize("which", FLAGS[1:])
def test_accumulating_passes_flags(env, which):
    _accumulated(env, "44x27m", (3, 5), 11, flags=_flag(which))


# ---- 6. the adaptive step ---------------------------------------------------------------------
ADAPT = {**OPTS, "tol_q16": 512}   # (OPTS' 4096 stops every tile of this frame at min_spp)


@pytest.mark.parametrize("which", FLAGS)
def test_adaptive_steps(env, which):
    """rt_adapt_step over 44x27m until no tile is active.  The expected counts
    and halves are the oracle's alone: 64 one-sample mirror frames through the
    rule in Python ints (tests/test_gpu_adapt.py's simulate).  Step for step
    the per-tile counts and the resolved frame are equal under the three
    variants and equal the simulation's; the first step's frame is the mirror's
    8-spp frame.  Engaged: by the oracle's counts some listed tile stops at
    min_spp while listed tiles and overflowed tiles go on, so the active list
    of the later steps holds both kinds and is shorter than the frame's;
    rt_adapt_step returns the list's length, held to the oracle's counts."""
    flags = _flag(which)
    name = "44x27m"
    sc, cam, w, h = env.frames[name]
    counts_of = env.counts[name].reshape(4, 6)
    ones = [mirror_ints(name, sc, cam, w, h, k, SEED, flags) for k in range(ADAPT["max_spp"])]
    counts, h0, h1 = simulate(ones, **ADAPT)
    print(counts)
    stopped, goes_on = counts == ADAPT["min_spp"], counts > ADAPT["min_spp"]
    assert (stopped & (counts_of >= 1) & (counts_of <= 14)).any()
    assert (goes_on & (counts_of >= 1) & (counts_of <= 14)).any() and (goes_on & (counts_of > 14)).any()
    p = B.params(w, h, spp=0, flags=flags)
    p.seed = SEED
    first = mirror(name, sc, cam, w, h, ADAPT["step_spp"], SEED, flags)

    def run(v):
        steps = []
        with uploaded(sc) as ds:
            q = B.params(w, h, spp=ADAPT["step_spp"], flags=flags)
            resolved(ds, q, v)
            ad = Ad(env, p, ADAPT, ds=ds)
            try:
                assert ad.active == 24
                while True:
                    rc = ad.step(cam)
                    assert rc >= 0, env.lib.rt_last_error()
                    if rc == 0:
                        break
                    steps.append((ad.counts(), ad.frame(flags), rc))   # (rc: the tiles the step traced)
                    assert len(steps) <= ADAPT["max_spp"] // ADAPT["step_spp"]
                halves, cnt = ad.read(), tuple(ad.counters())
            finally:
                ad.free()
        same((steps[0][1], ()), (first[0], ()), f"the first step's frame, variant {v}")
        px = np.array([[min(8, h - 8 * ty) * min(8, w - 8 * tx) for tx in range(6)] for ty in range(4)])
        assert cnt[1] == int((counts.astype(np.int64) * px).sum()), (v, cnt)
        assert (steps[0][0] == ADAPT["step_spp"]).all()
        for k, (c, _, traced) in enumerate(steps):
            spp = (k + 1) * ADAPT["step_spp"]
            assert np.array_equal(c, np.minimum(counts, spp)), (v, k)
            # the step's active list: the tiles whose final count it adds to
            assert traced == int((counts >= spp).sum()), (v, k, traced)
        assert steps[0][2] == 24 and 0 < steps[2][2] < 24, steps[2][2]
        assert np.array_equal(halves[0], h0) and np.array_equal(halves[1], h1), v
        return steps, cnt
    got = each_variant(run)
    for v in (LIST, DEFAULT):
        assert got[v][1] == got[WALK][1], (v, got[v][1], got[WALK][1])
        assert len(got[v][0]) == len(got[WALK][0]) == int(counts.max()) // ADAPT["step_spp"]
        for k, ((c, f, a), (cw, fw, aw)) in enumerate(zip(got[v][0], got[WALK][0])):
            assert np.array_equal(c, cw) and a == aw, (v, k)
            assert np.array_equal(f.view(np.uint32), fw.view(np.uint32)), (v, k)


# ---- 7. the budget's passes and the fused unit table ------------------------------------------
BEGIN = 5


@pytest.mark.parametrize("which", FLAGS)
def test_budget_passes_and_fused_trace(env, which):
    """A plan of multipliers 1 + t % 4 over 44x27m's tiles: 1, 2, 3, 4, 2 for the
    lists of 0, 1, 2, 5 and 14 bodies (tiles 0, 1, 2, 3, 9) and 1 and 4 for
    overflowed tiles (12 and 15).  H0 and H1 of rt_budget_trace and of
    rt_budget_trace_fused equal, integer for integer, the sums of the mirror's
    one-sample frames the contract names (block 2 j + h of a tile with
    multiplier m > j), with equal counters; and rt_launch_accum at a tile's own
    count, 2 m samples, gives that tile's H0 + H1.  Engaged: the multipliers
    read back are the plan's, the passes make 2 x 4 launches and the fused trace 2."""
    from rtclj import raytracing as R
    from rtclj._lib import rt_params, u64ptr
    flags = _flag(which)
    name = "44x27m"
    sc, cam, w, h = env.frames[name]
    torch = env.torch
    mult = (1 + np.arange(24) % 4).astype(np.uint32).reshape(4, 6)
    counts_of = env.counts[name]
    assert [int(counts_of[t]) for t in (0, 1, 2, 3, 9)] == [0, 1, 2, 5, 14] and counts_of[12] > 14 and counts_of[15] > 14
    assert {int(mult.ravel()[t]) for t in (0, 1, 2, 3, 9, 12, 15)} == {1, 2, 3, 4}
    m_px = per_pixel(mult, h, w)[..., None]
    one = [mirror_ints(name, sc, cam, w, h, BEGIN + b, SEED, flags) for b in range(8)]
    want = [sum(np.where(m_px > j, one[2 * j + half], np.uint64(0)) for j in range(4)) for half in (0, 1)]

    def run(v):
        with uploaded(sc) as ds:
            resolved(ds, B.params(w, h, spp=2, flags=flags), v)
            d_raw = torch.from_numpy(mult.astype(np.int32).reshape(-1)).cuda()
            got = {}
            for fused in (False, True):
                with R.Budget(ds, w, h, max_depth=DEPTH, seed=SEED, flags=flags, half_spp=1, max_mult=4) as bd:
                    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    bd.plan_mult(d_raw.data_ptr())
                    assert np.array_equal(bd.mult(), mult)
                    assert bd.trace(ds, cam, sample_begin=BEGIN, d_counters=cnt.data_ptr(), fused=fused) == (2 if fused else 8)
                    torch.cuda.synchronize()
                    h0, h1 = bd.halves()
                    got[fused] = (h0, h1, tuple(cnt.cpu().tolist()))
                assert np.array_equal(h0, want[0]) and np.array_equal(h1, want[1]), (v, fused)
            assert got[True][2] == got[False][2] and got[True][2][1] == int((m_px[..., 0] * 2).sum()), (v, got[True][2])
            # rt_launch_accum at each tile's own count
            for m in (1, 2, 3, 4):
                p = rt_params(width=w, height=h, row_begin=0, row_end=h, spp=2 * m, max_depth=DEPTH, seed=SEED,
                              sample_begin=BEGIN, flags=flags)
                acc = C.c_void_p()
                assert env.lib.rt_accum_create(ds, C.byref(p), C.byref(acc)) == 0, env.lib.rt_last_error()
                try:
                    assert env.lib.rt_launch_accum(ds, C.byref(cam), C.byref(p), acc, None, None) == 0, env.lib.rt_last_error()
                    whole = np.empty((h, w, 3), np.uint64)
                    assert env.lib.rt_accum_read(acc, u64ptr(whole), None) == 0
                finally:
                    env.lib.rt_accum_free(acc)
                sel = m_px[..., 0] == m
                assert sel.any() and np.array_equal((got[True][0] + got[True][1])[sel], whole[sel]), (v, m)
            return got[True][2]
    got = each_variant(run)
    assert got[WALK] == got[LIST] == got[DEFAULT], got


# ---- 8. a refit between frames ----------------------------------------------------------------
@pytest.mark.parametrize("which", FLAGS)
@pytest.mark.parametrize("knobs,spp", [({}, 7), (dict(RTCLJ_STEAL_MIN=1, **SHARING), 9)], ids=["default", "shared"])
def test_refit_between_frames(env, monkeypatch, knobs, spp, which):
    """40x24: a launch, rt_scene_update to moved(sc, 0), a launch,
    rt_scene_update back, a launch, on one stream.  The update rewrites the
    leaf records' bodies under list entries that keep their addresses: the
    spheres of tiles 3, 6, 9 and 12 leave their tiles' lists and enter the next
    tiles' (tile 13 goes from 13 bodies to 23: from the list to the walk, and
    back).  Each frame equals the mirror of the scene it shows and a fresh
    upload's frame.  Engaged: the two scenes' mirrors differ in the tiles whose
    lists differ."""
    _set(monkeypatch, knobs)
    flags = _flag(which)
    from rtclj import raytracing as R
    sc, cam, w, h = env.frames["40x24"]
    mv = B.moved(sc, 0)
    p = B.params(w, h, spp=spp, flags=flags)
    p.seed = SEED
    want = [mirror("40x24", sc, cam, w, h, spp, SEED, flags), mirror("40x24/moved0", mv, cam, w, h, spp, SEED, flags)]
    differ = (want[0][0] != want[1][0]).any(axis=-1)
    for t in (3, 4, 6, 7, 9, 12, 13):
        assert differ[8 * (t // 5):8 * (t // 5) + 8, 8 * (t % 5):8 * (t % 5) + 8].any(), t

    def run(v):
        with R.DeviceScene(sc) as d, uploaded(mv) as fresh:
            resolved(d.handle, p, v)
            for k, (scene, w_) in enumerate(((sc, want[0]), (mv, want[1]), (sc, want[0]), (mv, want[1]))):
                if k:
                    d.update(scene)
                same(launch(d.handle, cam, p), w_, f"variant {v} frame {k}")
            same(launch(fresh, cam, p), want[1], f"variant {v}, a fresh upload of the moved scene")
    each_variant(run)


# ---- 9. frames in flight ----------------------------------------------------------------------
@pytest.mark.parametrize("which", FLAGS)
def test_frames_in_flight(env, which):
    """rt_render_submit .. rt_render_wait: both scenes' frames submitted twice
    before any is waited for, waited for in reverse order; each equals its
    mirror, statistics included.  Engaged: four frames were in flight at once
    (four handles held unwaited)."""
    from rtclj import raytracing as R
    flags = _flag(which)
    jobs = []
    for name, spp in (("40x24", 9), ("44x27m", 24), ("40x24", 40), ("44x27m", 7)):
        sc, cam, w, h = env.frames[name]
        jobs.append((name, sc, cam, w, h, spp, mirror(name, sc, cam, w, h, spp, SEED, flags)))

    def run(v):
        with uploaded(jobs[0][1]) as ds:
            resolved(ds, B.params(40, 24, spp=9, flags=flags), v)
        frames = [R.render_async(sc, cam, w, h, spp=spp, max_depth=DEPTH, seed=SEED, n_devices=1, flags=flags)
                  for _, sc, cam, w, h, spp, _ in jobs]
        assert len(frames) == 4
        for k in reversed(range(4)):
            st = {}
            got = frames[k].wait(stats=st)
            same((got, (st["segments"], st["samples"])), jobs[k][6], f"variant {v} frame {k}")
    each_variant(run)
    env.lib.rt_cache_clear()


# ---- 10. the lists were used ------------------------------------------------------------------
@pytest.mark.parametrize("knobs,spp", [(dict(RTCLJ_STEAL_MIN=1, **SHARING), 40), (dict(RTCLJ_SPLIT=5), 40),
                                       (dict(RTCLJ_COMPACT=16, RTCLJ_SPLIT=1), 3)], ids=["shared", "split", "drained"])
def test_the_lists_were_used(env, monkeypatch, knobs, spp):
    """The statistics build's variant 31 (22 with wave-level counters) under one
    knob set of items 1, 2 and 3: its frame is variant 30's and the mirror's,
    and rt_debug_stats_ext shows prelude trips and list passes, with
    test_gpu_body_list.py's inequalities (a pass tests four bodies or two, an
    exact step belongs to a tested body).  A statistics variant never shares
    its tiles (trace.hip: the launch's `steal` excludes them), so the shared
    case runs whole unshared tiles there and no bound on the helpers' trips
    can be asserted; the drained case reads the drain checks, which show that
    its waves' batches were spent while they held paths (the gate's last
    clause), not that a wave posted: nothing counts the posts."""
    from rtclj import raytracing as R
    from rtclj._lib import check, diag_lib
    _set(monkeypatch, knobs)
    d = diag_lib()
    for name in B.MODE_FRAMES:
        sc, cam, w, h = env.frames[name]
        want = mirror(name, sc, cam, w, h, spp, SEED)
        got = {}
        old = d.rt_set_variant(WALK)
        assert old >= 0
        try:
            for v in (WALK, 31):
                assert d.rt_set_variant(v) >= 0, v
                check(d.rt_debug_stats((C.c_uint64 * 32)()))   # clear
                st = {}
                out = R.render(sc, cam, w, h, spp=spp, max_depth=DEPTH, seed=SEED, n_devices=1, stats=st, library=d)
                dbg = (C.c_uint64 * 40)()
                check(d.rt_debug_stats_ext(dbg, 40))
                got[v] = (out, (st["segments"], st["samples"])), [int(x) for x in dbg]
        finally:
            d.rt_set_variant(old)
        same(got[WALK][0], want, f"{name}: variant 30 of the statistics build")
        same(got[31][0], want, f"{name}: variant 31")
        s = got[31][1]
        trips, lanes, passes, exacts, bodies = s[27], s[28], s[29], s[30], s[32]
        print(name, dict(trips=trips, lanes=lanes, passes=passes, exacts=exacts, bodies=bodies, claims=s[25], drains=s[26]))
        assert trips > 0 and passes > 0
        assert 0 < 2 * passes <= bodies <= 4 * passes and exacts <= bodies
        assert passes <= s[12] and exacts <= s[13] and all(x == 0 for x in s[33:])
        # every sample of a listed tile starts in a trip: at most 64 lanes a trip
        listed_px = int(per_pixel((env.counts[name] <= 14).reshape(-1, (w + 7) // 8), h, w).sum())
        assert lanes == listed_px * spp and trips >= lanes / 64, (lanes, listed_px * spp, trips)
        assert got[WALK][1][27] == 0 and got[WALK][1][32] == 0
        if "RTCLJ_COMPACT" in knobs:
            assert s[26] > 0


# ---- 11. path export --------------------------------------------------------------------------
def _export_stats(env, ds):
    st = (C.c_uint64 * 2)()
    assert env.lib.rt_export_stats(ds, C.c_void_p(env.stream.cuda_stream), st) == 0
    return int(st[0]), int(st[1])


def _exported_frames(env, spps, flags=0):
    """Both frames at each spp, twice on one stream of a fresh upload, each
    launch against the mirror -> {(name, spp): {variant: (exporting launches, records)}}."""
    out = {}
    for name in B.MODE_FRAMES:
        sc, cam, w, h = env.frames[name]
        for spp in spps:
            p = B.params(w, h, spp=spp, flags=flags)
            p.seed = SEED
            want = mirror(name, sc, cam, w, h, spp, SEED, flags)

            def run(v):
                with uploaded(sc) as ds:
                    resolved(ds, p, v)
                    for k in range(2):
                        same(launch(ds, cam, p, env.stream), want, f"{name} {spp} spp variant {v} launch {k}")
                    return _export_stats(env, ds)
            out[(name, spp)] = each_variant(run)
    return out


def _check_export(got, every):
    """Variant 30 has no sweep: its launches export nothing, so its frame is
    the unexported one that 22's and the default's equal through the mirror.
    Under 22 and the default both launches exported; records were written in
    every case (`every`), or in some case of the knob set."""
    for v in (LIST, DEFAULT):
        print(v, {k: by[v] for k, by in got.items()})
        assert all(by[WALK] == (0, 0) and by[v][0] == 2 for by in got.values()), (v, got)
        recs = [by[v][1] for by in got.values()]
        assert all(r > 0 for r in recs) if every else sum(recs) > 0, (v, recs)


@pytest.mark.parametrize("knobs", [dict(RTCLJ_SPLIT=2), dict(RTCLJ_SPLIT=5), dict(RTCLJ_SPLIT=5, RTCLJ_EXPORT_LIM=16)],
                         ids=lambda k: "-".join(f"{n[6:].lower()}{v}" for n, v in k.items()))
def test_path_export(env, monkeypatch, knobs):
    """RTCLJ_EXPORT=1 on split launches: a wave of the list's kernel whose
    batches are spent and which holds at most RTCLJ_EXPORT_LIM paths (default
    64: any) writes them out as records and leaves -- a camera sample the gate
    had deferred and not yet started would be lost there -- and the sweep runs
    the records into the split sums.  Engaged: rt_export_stats counts both
    launches and, at the default limit, records in every case (at limit 16, in
    some case); under variant 30 the knob exports nothing."""
    _set(monkeypatch, {"RTCLJ_EXPORT": 1, **knobs})
    _check_export(_exported_frames(env, (7, 40)), every="RTCLJ_EXPORT_LIM" not in knobs)


@pytest.mark.parametrize("which", FLAGS[1:])
def test_path_export_flags(env, monkeypatch, which):
    _set(monkeypatch, dict(RTCLJ_EXPORT=1, RTCLJ_SPLIT=5))
    _check_export(_exported_frames(env, (7, 40), flags=_flag(which)), every=True)
