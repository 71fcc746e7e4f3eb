"""A Python restatement of the phases of k_td_lzw (csrc/tiff_decode.hip), not of the host decoder's loop: one batch of 64
codes at a time -- codes at closed-form bit offsets, the search for Clear / EOI / the end of the input / a code above the
table's fill level, the length recurrence, the prefix sum, the sources of every copy, the staged bytes and their flush.
Every index the kernel forms from file bytes is formed here too and asserted to be in range, so a hostile stream is seen
by these assertions on the CPU before it reaches a GPU.  tests/test_tiff_decode_cpu.py holds it against
lars_h_tiff_lzw_decode, the specification."""
PCAP = 3840          # TD_PCAP
STAGE = 4096         # TD_STAGE
CLEAR, EOI, FIRST = 256, 257, 258
LANES = 64


def bits_before(i):
    a = min(i, 254)
    b = 0 if i < 254 else min(i - 254, 512)
    c = 0 if i < 766 else min(i - 766, 1024)
    d = 0 if i < 1790 else i - 1790
    return 9 * a + 10 * b + 11 * c + 12 * d


def width_of(i):
    return 9 if i <= 253 else 10 if i <= 765 else 11 if i <= 1789 else 12


def new_events():
    """What decode() records about the paths a stream takes, for tests that assert their coverage: ``max_L`` the longest string,
    ``max_i`` the largest index of a decoded code in its segment, ``stage_full`` batches cut because the stage was full,
    ``pcap_batches`` batches begun with seg_i >= PCAP, ``totals`` the bytes of every batch, ``dep_b`` the kinds of second
    dependency seen ("self": code j + 1 is the copying code itself, KwKwK; "lane0": j is the last code in front of the batch,
    so the copy's source starts in the chunk buffer and ends in the stage; "inside": j + 1 is a lower lane; "none": both are
    in front of the batch), ``fill_lanes`` / ``next_lanes`` / ``clear_lanes`` / ``eoi_lanes`` the lanes at which the fill-level
    code, an entry with j + 1 == seg_i, a Clear and an EOI that ended a batch were seen, ``straddle_L`` the longest "lane0"
    copy, ``rounds`` the most copy rounds a batch took, ``first_at`` the indices i at which a batch ended in Clear or EOI."""
    return dict(max_L=0, max_i=-1, stage_full=0, pcap_batches=0, totals=set(), dep_b=set(), fill_lanes=set(), next_lanes=set(),
                clear_lanes=set(), eoi_lanes=set(), straddle_L=0, rounds=0, first_at=set(), batches=0)


def decode(src, ndst, events=None):
    """(bytes produced, bad): what the kernel leaves in produced[k] / bad[k] and in the chunk buffer for a stream ``src`` and a
    chunk of ``ndst`` bytes (ndst >= 1).  ``events``: a new_events() record to fill in."""
    ev = events if events is not None else new_events()
    src = bytes(src)
    cnt = len(src)
    assert ndst >= 1
    nbits = cnt * 8
    dst = bytearray(ndst)
    P = [None] * PCAP
    seg_bit, seg_i, op, err = 0, 0, 0, 0
    last_pos = -1
    while True:
        pos = seg_bit + bits_before(seg_i)
        assert pos > last_pos, "a batch that did not move on in the stream"
        last_pos = pos
        stage, when, owner = [None] * STAGE, [0] * STAGE, [0] * STAGE
        code, avail, term, wrong, idx = [0] * LANES, [False] * LANES, [False] * LANES, [False] * LANES, [0] * LANES
        for lane in range(LANES):
            i = idx[lane] = seg_i + lane
            at = seg_bit + bits_before(i)
            w = width_of(i)
            avail[lane] = at + w <= nbits
            if avail[lane]:
                byte = at >> 3
                assert 0 <= byte < cnt
                v = src[byte] << 16
                if byte + 1 < cnt:
                    v |= src[byte + 1] << 8
                if byte + 2 < cnt:
                    v |= src[byte + 2]
                shift = 24 - (at & 7) - w
                assert 0 <= shift
                code[lane] = (v >> shift) & ((1 << w) - 1)
            term[lane] = (not avail[lane]) or code[lane] in (CLEAR, EOI)
            wrong[lane] = (not term[lane]) and code[lane] >= FIRST and code[lane] - FIRST > i - 1
        n_term = term.index(True) if True in term else 64
        n_wrong = wrong.index(True) if True in wrong else 64
        ndata = min(n_term, n_wrong)
        if seg_i < PCAP:
            P[seg_i] = op
        else:
            ev["pcap_batches"] += 1
        ev["batches"] += 1
        # lengths
        L, need = [0] * LANES, [False] * LANES
        for lane in range(ndata):
            L[lane] = 1
            if code[lane] >= FIRST:
                j = code[lane] - FIRST
                assert 0 <= j <= idx[lane] - 1 and j + 1 < PCAP
                if j >= seg_i:
                    need[lane] = True
                    assert 0 <= j - seg_i < lane
                else:
                    assert P[j] is not None and P[j + 1] is not None
                    L[lane] = P[j + 1] - P[j] + 1
        rounds = 0
        while any(need):
            known = [not n for n in need]
            for lane in range(ndata):
                if need[lane]:
                    jl = code[lane] - FIRST - seg_i
                    if known[jl]:
                        L[lane], need[lane] = L[jl] + 1, False
            rounds += 1
            assert rounds <= 64
        assert all(1 <= L[lane] <= 3839 for lane in range(ndata))
        incl, run = [0] * LANES, 0
        for lane in range(LANES):
            run += L[lane]
            incl[lane] = run
        start = [op + incl[lane] - L[lane] for lane in range(LANES)]
        end = [op + incl[lane] for lane in range(LANES)]
        stop = [lane < ndata and ((idx[lane] >= 1 and end[lane] >= ndst) or (idx[lane] == 0 and start[lane] >= ndst)) for lane in range(LANES)]
        n_stop = stop.index(True) + 1 if True in stop else 65
        n_stage = sum(1 for lane in range(ndata) if incl[lane] <= STAGE)
        nproc = min(ndata, n_stop, n_stage)
        assert nproc >= 1 or ndata == 0
        ev["stage_full"] += n_stage < min(ndata, n_stop)
        for lane in range(nproc):
            ev["max_L"], ev["max_i"] = max(ev["max_L"], L[lane]), max(ev["max_i"], idx[lane])
            if code[lane] - FIRST == idx[lane] - 1:
                ev["fill_lanes"].add(lane)
            if code[lane] - FIRST + 1 == seg_i:
                ev["next_lanes"].add(lane)
        for lane in range(nproc):
            if idx[lane] < PCAP:
                P[idx[lane]] = start[lane]
        # bytes, in rounds of lanes whose sources are written
        todo = [lane < nproc for lane in range(LANES)]
        rounds = 0
        while any(todo):
            done = [not t for t in todo]
            for lane in range(nproc):
                if not todo[lane]:
                    continue
                base = start[lane] - op
                if code[lane] < FIRST:
                    assert 0 <= base < STAGE
                    stage[base], when[base], owner[base] = code[lane], rounds, lane
                    todo[lane] = False
                    continue
                j = code[lane] - FIRST
                inside = j >= seg_i
                jl = j - seg_i if inside else 0
                dep_a = jl if inside else -1
                lane_b = (jl + 1 if inside else 0)
                dep_b = lane_b if (j + 1 >= seg_i and lane_b != lane) else -1
                assert dep_a < lane and dep_b < lane
                kind = "self" if lane_b == lane and j + 1 >= seg_i else "none" if dep_b < 0 else "inside" if inside else "lane0"
                if (dep_a >= 0 and not done[dep_a]) or (dep_b >= 0 and not done[dep_b]):
                    continue
                assert j < PCAP and P[j] is not None
                srcpos = P[j]
                ev["dep_b"].add(kind)
                if kind == "lane0":
                    ev["straddle_L"] = max(ev["straddle_L"], L[lane])
                for t in range(L[lane]):
                    s = srcpos + t
                    if s < op:
                        assert 0 <= s < ndst
                        b = dst[s]
                    else:
                        assert 0 <= s - op < STAGE and stage[s - op] is not None, "a source byte that is not written yet"
                        # the lanes of a round run side by side: a byte of another lane counts only from the round before
                        assert owner[s - op] == lane or when[s - op] < rounds, "a source byte another lane writes in this round"
                        b = stage[s - op]
                    assert 0 <= base + t < STAGE
                    stage[base + t], when[base + t], owner[base + t] = b, rounds, lane
                todo[lane] = False
            rounds += 1
            assert rounds <= 64
        ev["rounds"] = max(ev["rounds"], rounds)
        total = incl[nproc - 1] if nproc > 0 else 0
        ev["totals"].add(total)
        assert total <= STAGE
        for q in range(total):
            assert stage[q] is not None
            if op + q < ndst:
                dst[op + q] = stage[q]
        if nproc > 0 and nproc == n_stop:
            op = ndst
            break
        op += total
        assert op < ndst or (seg_i == 0 and nproc <= 1 and op == ndst)       # only a first literal fills the chunk and goes on (to a Clear, say)
        seg_i += nproc
        if nproc < ndata:
            continue
        if n_wrong < n_term:
            err = 1
            break
        if n_term == 64:
            continue
        if avail[n_term]:
            ev["eoi_lanes" if code[n_term] == EOI else "clear_lanes"].add(n_term)
            ev["first_at"].add(seg_i)
        if (not avail[n_term]) or code[n_term] == EOI:
            break
        seg_bit += bits_before(seg_i) + width_of(seg_i)
        seg_i = 0
        P = [None] * PCAP                                                    # the kernel keeps the old offsets; reading one is an error here
    return bytes(dst[:op]), err
