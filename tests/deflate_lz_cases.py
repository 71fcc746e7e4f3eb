"""The byte strings the tests of the Deflate coder's string matching share (tests/test_deflate_lz_cpu.py judges the model on them,
tests/test_gpu_deflate_lz.py the device against the model).  Every string is one TIFF strip: encode_tiff(uint8 [1, n],
rows_per_strip=1, compression="deflate") codes exactly these bytes.  All seeded; nothing here touches the device."""
import functools

import numpy as np

import deflate_lz_model as lm

SEG = lm.SEG


def _rng(seed):
    return np.random.default_rng(seed)


def _values(seed, n, k):
    """n random bytes over the k values 0 .. k-1."""
    return _rng(seed).integers(0, k, n, dtype=np.uint8).tobytes()


def periodic(p, n, seed):
    unit = _rng(seed).permutation(256)[:p].astype(np.uint8).tobytes() if p <= 256 else _values(seed, p, 256)
    return (unit * (n // p + 1))[:n]


def far_word():
    """32768 bytes: a 4-byte word at 0 and again at n - 4, between them 509 random bytes over and over.  The filler's 4-byte words
    fill few hash buckets, so the table still holds position 0 when the last tile looks the word up: distance 32764, 13 extra bits,
    and the match ends on the segment's last byte."""
    fill = periodic(509, SEG - 8, 31)
    used = {lm.hash4(fill, j) for j in range(len(fill) - 3)}
    word = next(w for w in (bytes([200 + a, 210 + b, 220 + c, 230 + d]) for a in range(9) for b in range(9) for c in range(9) for d in range(9))
                if lm.hash4(w, 0) not in used)
    data = word + fill + word
    assert lm.parse(data)[-1] == (4, SEG - 4)
    return data


def same_hash():
    """Two different 4-byte words of one hash, the second at a tile's first position: its candidate has length 0."""
    a = bytes([1, 2, 3, 4])
    b = next(w for w in (bytes([9, x, y, 7]) for x in range(256) for y in range(256)) if lm.hash4(w, 0) == lm.hash4(a, 0))
    fill = bytes(range(4, 256))                               # 252 bytes, no repeats
    data = a + fill + b + bytes(range(100, 140))
    assert len(a + fill) == lm.TILE and lm.candidates(data)[lm.TILE] == 0 and lm.best_match(data, lm.candidates(data), lm.TILE) == (0, 0)
    return data


LENGTH_BASES = (4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DISTANCE_BASES = (5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
                  16385, 24577)


def planted():
    """A full segment of bytes over 64 values with copies planted at the first position of a tile: every distance symbol from 4 on and
    every length symbol from 258 on, each at its base value, and a 3-byte repeat."""
    seg = bytearray(_values(41, SEG, 64))
    plants, taken = [], set()
    for i, dist in enumerate(DISTANCE_BASES + tuple(300 + 37 * k for k in range(58))):
        length = LENGTH_BASES[i % len(LENGTH_BASES)]
        tile = max(2, -(-dist // lm.TILE))
        while tile in taken or (length > 250 and tile + 1 in taken):
            tile += 1
        taken.update((tile, tile + 1) if length > 250 else (tile,))
        assert tile * lm.TILE + length < SEG
        plants.append((tile * lm.TILE, length, dist))
    for j, length, dist in sorted(plants):
        seg[j:j + length] = seg[j - dist:j - dist + length]
        seg[j + length] = seg[j - dist + length] ^ 0x80      # a value the filler never has: the match ends here
    seg[100:107] = bytes([201, 202, 203, 201, 202, 203, 204])    # literal x3, (3, 3), literal
    return bytes(seg)


def fibonacci():
    """Groups (x, x, x, y): x < 32 with frequencies like Fibonacci numbers, y a random byte >= 128, so that few 4-byte words come
    twice and the frequent x stay literals: the literal/length tree is deeper than 15 before the limit.  Copies of 100 bytes at the
    first position of every fourth tile put length symbols into that tree and make the matched block the shortest."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    rng = _rng(55)
    x = rng.permutation(np.repeat(np.arange(len(fib) + 1, dtype=np.uint8), fib + [3 * SEG // 4 - sum(fib)]))
    seg = np.empty(SEG, np.uint8)
    seg[0::4], seg[1::4], seg[2::4] = x[0::3], x[1::3], x[2::3]
    seg[3::4] = rng.integers(128, 256, SEG // 4, dtype=np.uint8)
    seg = bytearray(seg.tobytes())
    for tile in range(8, SEG // lm.TILE, 4):
        j = tile * lm.TILE
        dist = 4 * int(rng.integers(100, j // 4))
        seg[j:j + 100] = seg[j - dist:j - dist + 100]
    return bytes(seg)


def skewed_copies():
    """Literal frequencies like Fibonacci numbers, and at the first position of every tile
    from the 16th on a copy of 30 .. 60 bytes whose distance symbol is 10 + i with probability about 2^-i: both trees are skewed.
    One copy is alone in its length symbol (140 bytes) and in its distance symbol (the farthest): the widest token."""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= SEG:
        fib.append(fib[-1] + fib[-2])
    rng = _rng(51)
    body = rng.permutation(np.repeat(np.arange(len(fib), dtype=np.uint8), fib))
    seg = bytearray(body.tobytes() + bytes(100 + v for v in _values(52, SEG - body.size, 4)))
    for tile in range(16, SEG // lm.TILE):
        j = tile * lm.TILE
        sym = min(10 + int(rng.geometric(0.5)) - 1, 27)
        lo = (DISTANCE_BASES + (SEG,))[sym - 4]
        dist = min(lo + int(rng.integers(0, 8)), j)
        length = int(rng.integers(30, 61))
        if tile == 120:
            dist, length = j - 3, 140
        seg[j:j + length] = seg[j - dist:j - dist + length]
        seg[j + length] = 255
    return bytes(seg)


@functools.lru_cache(maxsize=None)
def byte_cases():
    """{name: bytes}: the exact-byte cases."""
    cases = {}
    for n in (1, 2, 3, 4, 5, 259, 260, 261, 262, 263):
        cases[f"equal{n}"] = bytes([77]) * n
    for p, n in ((1, 700), (2, 700), (3, 700), (4, 700), (5, 700), (7, 700), (255, 1500), (256, 1500), (257, 1500), (4096, 3 * 4096 + 50)):
        cases[f"period{p}"] = periodic(p, n, 60 + p)
    cases["far_word"] = far_word()
    for n in (32767, 32768, 32769, 65536):
        cases[f"zeros{n}"] = bytes(n)
    head = periodic(700, SEG + 200, 71)
    cases["repeat_across_segments"] = head[:SEG - 40] + head[1000:1080] + head[SEG + 40:]     # 40 bytes of the copy in each segment
    cases["same_hash"] = same_hash()
    cases["random"] = _values(81, SEG + 900, 256)
    cases["random16"] = _values(82, SEG + 900, 16)
    cases["planted"] = planted()
    cases["fibonacci"] = fibonacci()
    cases["skewed_copies"] = skewed_copies()
    return cases


@functools.lru_cache(maxsize=None)
def streams():
    """{name: (the model's stream, the model's record)} of byte_cases(), computed once."""
    out = {}
    for name, data in byte_cases().items():
        rec = {}
        out[name] = (lm.stream(data, rec), rec)
    return out
