"""Inputs for the value-window pre-pass of uint16 tiles, built FROM the model (tests/u16_window_model.py): every constructor asks
where the subsample looks and where the predicted window ends, and places values in the pixels the subsample does not see so that
the four order statistics np.percentile reads land where the case wants them.  Each case states the verdict it was built for
(per tile and channel: which of the four ranks lie inside their window); tests/test_u16_windows_cpu.py holds the constructors to
their claims before a GPU sees the inputs, tests/test_gpu_u16_windows.py runs them."""
import functools

import numpy as np

import u16_window_model as model

H, W = 512, 768                    # 393216 pixels: two sampled stretches (pixels 0..4095 and 262144..266239)
IN = (True, True, True, True)
A, MID, C = 10000, 30000, 50000    # the three levels of the designed channels


class Case:
    """tiles uint16[ntiles][h][w][3]; claims[tile][channel] = the four verdicts the tile was built for; planes: the GPU test also
    runs process() with an NDVI plane on it; repeat: the batch is these tiles repeated up to that many (case h)."""

    def __init__(self, name, tiles, claims, planes=False, repeat=None, expect=None):
        self.name, self.tiles, self.claims, self.planes, self.repeat = name, np.ascontiguousarray(tiles), claims, planes, repeat
        self.expect = expect or {}             # {(tile, channel, mark): percentile} stated by the case

    @property
    def flags(self):
        return [int(not all(all(v) for v in tile)) for tile in self.claims]


# ---- building blocks ------------------------------------------------------------------------------------------------------------
def compose(npix, seen, hidden):
    """A channel of npix samples: `seen` in the pixels the subsample reads (in its order), `hidden` in all others in ascending pixel
    order -- so the npix & 3 tail pixels, which are never sampled, take the last entries of `hidden`."""
    pos = model.sampled_pixels(npix)
    assert len(seen) == pos.size and len(hidden) == npix - pos.size, (len(seen), pos.size, len(hidden), npix - pos.size)
    ch = np.empty(npix, np.int64)
    mask = np.zeros(npix, bool)
    mask[pos] = True
    ch[pos] = seen
    ch[~mask] = hidden
    assert ch.min() >= 0 and ch.max() <= 65535
    return ch.astype(np.uint16)


def nseen(npix):
    return model.sampled_pixels(npix).size


def levels(n, low, mid, high, rng, low_part=0.10, high_part=0.10):
    """What the subsample sees of a designed channel: low_part of its n samples from `low`, high_part from `high`, the rest `mid`.
    low / high: a value, or (first, last) for values spread evenly over that range."""
    nl, nh = int(round(n * low_part)), int(round(n * high_part))

    def part(spec, count):
        if isinstance(spec, tuple):
            return np.linspace(spec[0], spec[1], count).astype(np.int64)
        return np.full(count, spec, np.int64)
    return rng.permutation(np.concatenate([part(low, nl), np.full(n - nl - nh, mid, np.int64), part(high, nh)]))


def seen_windows(npix, seen):
    """The windows the model predicts from `seen` alone (they depend on nothing else)."""
    return model.windows(compose(npix, seen, np.zeros(npix - len(seen), np.int64)))


def _low_counts(seen, r, p, q, fill, pad):
    """How many hidden samples of value `fill` (< p; None: none), p and q make sorted[r] = p and sorted[r + 1] = q, given that the
    seen samples hold nothing strictly between p and q.  pad: copies beyond the need (0: the run of q ends at rank r + 1 when p == q)."""
    lt, le = int((seen < p).sum()), int((seen <= p).sum())
    if p == q:
        a = 0 if fill is None else r - lt
        b = r + 2 + pad - (a + le)
        if fill is not None and b < 0:
            a, b = a + b, 0
        out = {p: b}
    else:
        b = max(1 - (le - lt), 0) if fill is not None else r + 1 - le
        a = 0 if fill is None else r + 1 - le - b
        out = {p: b, q: max(1 + pad - int((seen == q).sum()), 0)}
    assert a >= 0 and all(v >= 0 for v in out.values()), (a, out)
    if fill is not None:
        assert fill < p
        out[fill] = out.get(fill, 0) + a
    return out


def design(npix, seen, low, high, rng, fill_lo=None, fill_hi=None, mid=MID, pad=3, tail_smallest=0):
    """A channel whose subsample is `seen` and whose order statistics at the 2 % mark's two ranks are low = (p, q) and at the 98 %
    mark's high = (s, t): copies of those values (and of fill_lo < p / fill_hi > t where given, else more copies of p / t) go into the
    hidden pixels, `mid` fills the rest.  tail_smallest: that many of the smallest hidden samples go into the last hidden pixels (the
    ragged tail)."""
    seen = np.asarray(seen, np.int64)
    (r0, _, r1, _), _ = model.ranks(npix)
    counts = _low_counts(seen, r0, low[0], low[1], fill_lo, pad)
    mirrored = _low_counts(65535 - seen, npix - r1 - 2, 65535 - high[1], 65535 - high[0], None if fill_hi is None else 65535 - fill_hi, pad)
    for v, k in mirrored.items():
        counts[65535 - v] = counts.get(65535 - v, 0) + k
    nhidden = npix - seen.size
    rest = nhidden - sum(counts.values())
    assert rest >= 0, rest
    counts[mid] = counts.get(mid, 0) + rest
    hidden = np.concatenate([np.full(k, v, np.int64) for v, k in sorted(counts.items())])
    if tail_smallest:
        tail = hidden[:tail_smallest] - np.arange(1, tail_smallest + 1)          # smaller than every other sample, and distinct
        hidden = np.concatenate([rng.permutation(hidden[tail_smallest:]), tail])
    else:
        hidden = rng.permutation(hidden)
    ch = compose(npix, seen, hidden)
    assert model.order_statistics(ch) == [low[0], low[1], high[0], high[1]], (model.order_statistics(ch), low, high)
    return ch


def narrow(npix, base, rng):
    """A stationary, narrow channel: 40 adjacent values, every pixel drawn alike -- both windows hit."""
    return (base + rng.integers(0, 40, npix)).astype(np.uint16)


def tile_of(shape, channels):
    return np.stack([np.asarray(c, np.uint16).reshape(shape) for c in channels], axis=-1)


def gradient(shape, rng):
    """Case (a): row * 100 + noise.  The subsample sees a few rows at the top and a few in the middle, the marks lie elsewhere."""
    rows = np.arange(shape[0], dtype=np.int64)[:, None, None] * 100
    return (rows + rng.integers(0, 100, shape + (3,))).astype(np.uint16)


def straddle(npix, rng, side, step):
    """Case (b): the subsample sees 10 % at 10000, 80 % at 30000, 10 % at 50000; the hidden pixels hold exactly enough of the outer
    value that one rank of the pair is the outer value and its neighbour 30000 (step 0), or one more (step 1: both ranks inside)."""
    seen = levels(nseen(npix), A, MID, C, rng)
    low = (A, MID) if side == "low" and step == 0 else (A, A)
    high = (MID, C) if side == "high" and step == 0 else (C, C)
    pad = 0 if step else 3                         # step 1: ONE more than the straddle -- the run ends at the pair's second rank
    ch = design(npix, seen, low, high, rng, pad=pad)
    return ch


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def case_a():
    rng = np.random.default_rng(101)
    out = (False, False, False, False)
    return Case("a-hidden-tails", gradient((H, W), rng)[None], [(out, out, out)])


def case_b():
    npix = H * W
    tiles, claims, expect = [], [], {}
    for i, (side, step, want) in enumerate((("low", 0, (True, False, True, True)), ("low", 1, IN),
                                            ("high", 0, (True, True, False, True)), ("high", 1, IN))):
        rng = np.random.default_rng(200 + i)
        tiles.append(tile_of((H, W), [straddle(npix, rng, side, step), narrow(npix, 21000, rng), narrow(npix, 40000, rng)]))
        claims.append((want, IN, IN))
    expect[(0, 0, 0)] = 16000.0
    return Case("b-straddle", np.stack(tiles), claims, planes=True, expect=expect)


def case_c():
    """Decisive values on lo, on lo + wd - 1 (hits) and on lo + wd (flagged), at either mark; and with a channel whose two windows
    have different predicted widths, so that the width that counts is the widened one."""
    npix = H * W
    n = nseen(npix)
    tiles, claims = [], []
    rng = np.random.default_rng(300)
    seen = levels(n, A, MID, C, rng)
    (lo0, wd0), (lo1, wd1) = seen_windows(npix, seen)
    assert (lo0, wd0, lo1, wd1) == (9984, 48, 49984, 48)
    out2, out98 = (False, False, True, True), (True, True, False, False)
    placements = [
        # (low pair, high pair, fill_lo, fill_hi, verdict of channel 0)
        ((lo0, lo0), (lo1, lo1), 5000, 60000, IN),                                   # both marks on lo; rank == count below the window
        ((lo0 + wd0 - 1,) * 2, (lo1 + wd1 - 1,) * 2, 5000, 60000, IN),               # both on the last value
        ((lo0 + wd0,) * 2, (C, C), 5000, None, out2),                                # 2 % on lo + wd
        ((A, A), (lo1 + wd1,) * 2, None, 60000, out98),                              # 98 % on lo + wd
        ((lo0 - 1,) * 2, (lo1 - 1,) * 2, 5000, 60000, (False,) * 4),                 # one below lo
        ((lo0 + wd0 - 1, lo0 + wd0), (lo1 - 1, lo1), 5000, 60000, (True, False, False, True)),   # the pairs straddle the edges
    ]
    for low, high, flo, fhi, want in placements:
        tiles.append(tile_of((H, W), [design(npix, seen, low, high, rng, flo, fhi), narrow(npix, 21000, rng), narrow(npix, 40000, rng)]))
        claims.append((want, IN, IN))
    # different predicted widths: the top of the subsample spreads over 50000..50150, the bottom sits on one value
    seen_w = levels(n, A, MID, (C, C + 150), rng)
    (wl0, ww0), (wl1, ww1) = seen_windows(npix, seen_w)
    assert wl0 == 9984 and ww0 == ww1 > 48, (wl0, ww0, wl1, ww1)       # own width 48, widened to the 98 % mark's
    for low, want in (((wl0 + ww0 - 1,) * 2, IN), ((wl0 + ww0,) * 2, out2), ((wl0 + 48,) * 2, IN)):
        mid_top = wl1 + ww1 // 2
        tiles.append(tile_of((H, W), [narrow(npix, 21000, rng), design(npix, seen_w, low, (mid_top, mid_top), rng, 5000, 60000),
                                      narrow(npix, 40000, rng)]))
        claims.append((IN, want, IN))
    return Case("c-window-edges", np.stack(tiles), claims)


def no_window_channel(npix, rng, which="low"):
    """One mark without a window (the subsample's ranks around it span more than 1024 values) beside a mark that has one.  The
    hidden pixels put the windowless mark's order statistics where the OTHER mark's width, measured from 0, would catch them."""
    n = nseen(npix)
    if which == "low":
        seen = levels(n, (0, 20000), MID, C, rng, low_part=0.05)
        ch = design(npix, seen, (20, 20), (C, C), rng)
        (l0, w0), (l1, w1) = model.windows(ch)
        assert w0 == 0 and l0 == 0 and w1 == 48 and 20 < w1
        return ch, (False, False, True, True)
    seen = levels(n, A, MID, (45000, 65000), rng, high_part=0.05)
    ch = design(npix, seen, (A, A), (65530, 65530), rng)
    (l0, w0), (l1, w1) = model.windows(ch)
    assert w1 == 0 and w0 == 48
    return ch, (True, True, False, False)


def case_d():
    """One channel only, rotated through the three; one mark only; one mark without a window."""
    npix = H * W
    n = nseen(npix)
    tiles, claims = [], []
    out = (False,) * 4
    for c in range(3):                                      # (a) in one channel, (b) in one channel
        rng = np.random.default_rng(400 + c)
        g = gradient((H, W), rng)
        chans = [narrow(npix, 21000 + 5000 * k, rng) for k in range(3)]
        chans[c] = g[..., c].ravel()
        tiles.append(tile_of((H, W), chans))
        claims.append(tuple(out if k == c else IN for k in range(3)))
        chans = [narrow(npix, 3000 + 9000 * k, rng) for k in range(3)]
        chans[c] = straddle(npix, rng, "low" if c != 1 else "high", 0)
        tiles.append(tile_of((H, W), chans))
        claims.append(tuple(((True, False, True, True) if c != 1 else (True, True, False, True)) if k == c else IN for k in range(3)))
    rng = np.random.default_rng(410)
    seen = levels(n, A, MID, C, rng)
    miss2 = design(npix, seen, (12000, 12000), (C, C), rng, 5000, None)            # 2 % mark outside, 98 % inside
    miss98 = design(npix, seen, (A, A), (48000, 48000), rng, None, 60000)          # and the reverse
    tiles.append(tile_of((H, W), [narrow(npix, 21000, rng), miss2, narrow(npix, 40000, rng)]))
    claims.append((IN, (False, False, True, True), IN))
    tiles.append(tile_of((H, W), [narrow(npix, 21000, rng), narrow(npix, 40000, rng), miss98]))
    claims.append((IN, IN, (True, True, False, False)))
    for which, c in (("low", 0), ("high", 2)):
        ch, want = no_window_channel(npix, rng, which)
        chans = [narrow(npix, 21000 + 5000 * k, rng) for k in range(3)]
        chans[c] = ch
        tiles.append(tile_of((H, W), chans))
        claims.append(tuple(want if k == c else IN for k in range(3)))
    return Case("d-one-channel", np.stack(tiles), claims, planes=True)


def case_e():
    """A mixed batch: hit / miss / hit / no window / hit / miss, the first and the last tile like no other."""
    npix = H * W
    rng = np.random.default_rng(500)
    out = (False,) * 4
    nowin, want_nowin = no_window_channel(npix, rng, "low")
    tiles = [
        tile_of((H, W), [narrow(npix, 1000 + 7000 * k, rng) for k in range(3)]),
        gradient((H, W), rng),
        tile_of((H, W), [straddle(npix, rng, "low", 1), narrow(npix, 21000, rng), straddle(npix, rng, "high", 1)]),
        tile_of((H, W), [narrow(npix, 33000, rng), nowin, narrow(npix, 52000, rng)]),
        tile_of((H, W), [narrow(npix, 60000 - 9000 * k, rng) for k in range(3)]),
        tile_of((H, W), [narrow(npix, 8000, rng), narrow(npix, 45000, rng), straddle(npix, rng, "high", 0)]),
    ]
    claims = [(IN, IN, IN), (out, out, out), (IN, IN, IN), (IN, want_nowin, IN), (IN, IN, IN), (IN, IN, (True, True, False, True))]
    return Case("e-mixed-batch", np.stack(tiles), claims, planes=True)


RAGGED = ((511, 513), (509, 513), (510, 513))      # npix & 3 == 3, 1, 2; each just above the window route's floor


def ragged_channel(shape, rng, with_tail):
    """Case (f): the npix & 3 tail pixels hold the channel's smallest samples, and the window's samples end exactly at the 2 % pair's
    second rank: counted with the tail both ranks are inside, without it the second one falls past the window's samples.
    with_tail False: the same but one sample fewer inside, i.e. a miss as built."""
    npix = shape[0] * shape[1]
    k = npix & 3
    seen = levels(nseen(npix), A, MID, C, rng)
    (lo0, wd0), _ = seen_windows(npix, seen)
    p = lo0 + wd0 - 1
    if with_tail:
        return design(npix, seen, (p, p), (C, C), rng, fill_lo=7, pad=0, tail_smallest=k)
    return design(npix, seen, (p, MID), (C, C), rng, fill_lo=7, pad=0, tail_smallest=k)


def case_f(shape):
    rng = np.random.default_rng(600 + shape[0])
    npix = shape[0] * shape[1]
    hit = tile_of(shape, [narrow(npix, 21000, rng), ragged_channel(shape, rng, True), narrow(npix, 40000, rng)])
    miss = tile_of(shape, [narrow(npix, 21000, rng), narrow(npix, 40000, rng), ragged_channel(shape, rng, False)])
    return [Case("f-ragged-%dx%d-hit" % shape, hit[None], [(IN, IN, IN)]),
            Case("f-ragged-%dx%d-miss" % shape, miss[None], [(IN, IN, (True, False, True, True))])]


def case_g():
    """The ends of the range, and channels whose two marks share one window."""
    npix = H * W
    n = nseen(npix)
    rng = np.random.default_rng(700)
    seen = levels(n, 0, MID, 65535, rng)
    assert seen_windows(npix, seen) == ((0, 32), (65504, 32))
    ends0 = design(npix, seen, (0, 0), (65535, 65535), rng)
    ends1 = design(npix, seen, (15, 15), (65504, 65504), rng)                      # 65504 = 65536 - wd
    constant = np.full(npix, 4242, np.uint16)
    adjacent = (30000 + rng.integers(0, 2, npix)).astype(np.uint16)                # both values in one bin of the subsample
    across = (30015 + rng.integers(0, 2, npix)).astype(np.uint16)                  # ... and in two
    # a wide window at the bottom beside a narrow one at the very top: widened, the top one reaches past 65535
    # (65504 + wd - 65536 values from 0 upwards are 16-bit neighbours of its last values: the hidden pixels hold thousands of them)
    seen_w = levels(n, (0, 2000), MID, 65535, rng)
    (l0, w0), (l1, w1) = seen_windows(npix, seen_w)
    assert 3 < l0 and l1 == 65504 and w1 == w0 > 32 and l1 + w1 - 65536 > 3
    past_top = design(npix, seen_w, (l0 + 100, l0 + 100), (65535, 65535), rng, fill_lo=3)
    beyond = design(npix, seen, (32, 32), (65503, 65503), rng)                     # one past either window
    tiles = [tile_of((H, W), [ends0, ends1, constant]), tile_of((H, W), [adjacent, across, past_top]),
             tile_of((H, W), [constant, beyond, adjacent])]
    return Case("g-range-ends", np.stack(tiles), [(IN, IN, IN), (IN, IN, IN), (IN, (False,) * 4, IN)])


H_SHAPE = (512, 513)               # 262656 pixels: 65 stretches, two of them sampled (the second one 128 quads long)


def smallest_two_in_flight():
    """(ntiles, why) of the smallest batch of H_SHAPE tiles in which k_u16_sample12 has two stretches in flight: more sampled
    stretches per tile than workgroups per tile."""
    npix = H_SHAPE[0] * H_SHAPE[1]
    for ntiles in range(1, 65536):
        grid_x, nsampled = model.launch_geometry(ntiles, npix)
        if nsampled > grid_x:
            return ntiles
    raise AssertionError("no batch of this shape reaches the branch")


def case_h():
    """Two sampled stretches in flight: a handful of distinct tiles repeated.  One of type (a); two whose second sampled stretch
    differs from the first so that one of the windows is predicted from the second stretch alone."""
    shape = H_SHAPE
    npix = shape[0] * shape[1]
    n = nseen(npix)
    assert n == 4096 + 512
    rng = np.random.default_rng(800)
    out = (False,) * 4
    second_high = np.concatenate([np.full(4096, A, np.int64), np.full(512, C, np.int64)])       # the top window is in the second stretch
    second_low = np.concatenate([np.full(4096, C, np.int64), np.full(512, A, np.int64)])        # the bottom window
    for seen in (second_high, second_low):
        assert seen_windows(npix, seen) == ((9984, 48), (49984, 48))
    tiles = [
        gradient(shape, rng),
        tile_of(shape, [design(npix, second_high, (A, A), (C, C), rng), narrow(npix, 21000, rng), design(npix, second_low, (A, A), (C, C), rng)]),
        tile_of(shape, [narrow(npix, 1000 + 7000 * k, rng) for k in range(3)]),
        tile_of(shape, [narrow(npix, 40000, rng), design(npix, second_low, (A, MID), (C, C), rng), design(npix, second_high, (A, A), (MID, C), rng)]),
        tile_of(shape, [design(npix, second_low, (A, A), (C, C), rng), design(npix, second_high, (A, A), (C, C), rng), narrow(npix, 5000, rng)]),
    ]
    claims = [(out, out, out), (IN, IN, IN), (IN, IN, IN), (IN, (True, False, True, True), (True, True, False, True)), (IN, IN, IN)]
    return Case("h-two-in-flight", np.stack(tiles), claims, repeat=smallest_two_in_flight())


@functools.lru_cache(maxsize=None)
def small_cases():
    """Cases (a) to (g): a few megabytes each."""
    cases = [case_a(), case_b(), case_c(), case_d(), case_e()]
    for shape in RAGGED:
        cases += case_f(shape)
    cases.append(case_g())
    return tuple(cases)


SMALL_NAMES = ("a-hidden-tails", "b-straddle", "c-window-edges", "d-one-channel", "e-mixed-batch") + tuple(
    "f-ragged-%dx%d-%s" % (s[0], s[1], k) for s in RAGGED for k in ("hit", "miss")) + ("g-range-ends",)


def small_case(name):
    return {c.name: c for c in small_cases()}[name]


def existing_ten_tiles():
    """The ten tiles of tests/test_gpu_batch.py::test_uint16_percentiles_one_pass_and_its_recount, built as that test builds them."""
    rng = np.random.default_rng(21)
    h, w = 512, 768
    ramp = (np.arange(h * w * 3, dtype=np.int64).reshape(h, w, 3) * 7919 % 65536).astype(np.uint16)
    return np.stack([
        rng.integers(0, 65536, (h, w, 3), dtype=np.uint16),
        np.clip(rng.normal(30000, 900, (h, w, 3)), 0, 65535).astype(np.uint16),
        np.full((h, w, 3), 4242, np.uint16),
        np.where(rng.random((h, w, 3)) < 0.03, 65535, 7).astype(np.uint16),
        (rng.integers(0, 4, (h, w, 3)) * 21845).astype(np.uint16),
        np.clip(rng.normal(255.6 * 50, 40, (h, w, 3)), 0, 65535).astype(np.uint16),
        ramp,
        (rng.integers(0, 4096, (h, w, 3)) * 16).astype(np.uint16),
        np.clip(rng.normal(800, 300, (h, w, 3)), 0, 4095).astype(np.uint16),
        np.where(rng.random((h, w, 3)) < 0.5, rng.integers(0, 65536, (h, w, 3)), 30000).astype(np.uint16),
    ])
