"""tests/jpegdec_np.py -- TEST INFRASTRUCTURE ONLY: the NumPy restatement of DESIGN.md section 4 "JPEG decoding".  `decode` is a plain sequential baseline
decoder (its own marker walk, entropy decoding over the unstuffed bytes, vectorised inverse DCT, upsampling and colour) that the host build of
csrc/y7t_jpegdec.h and the device kernels are compared with stage by stage; `sync_rounds` restates the self-synchronising scheme (a lane per subsequence of
stuffed bytes, runs of lanes, rounds inside a run and launches between runs) to count what a stream needs."""
import numpy as np

ZIG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Stream:
    """what the markers of a one-scan baseline file say"""

    def __init__(self, data):
        data = bytes(data)
        assert data[:2] == b"\xff\xd8"
        self.qt, self.huff, self.ri, pos = {}, {}, 0, 2
        while True:
            assert data[pos] == 0xFF
            m, ln = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
            seg = data[pos + 4:pos + 2 + ln]
            if m == 0xDB:
                while seg:
                    assert seg[0] >> 4 == 0
                    t = np.zeros(64, np.int64)
                    t[ZIG] = list(seg[1:65])
                    self.qt[seg[0] & 15], seg = t, seg[65:]
            elif m == 0xC4:
                while seg:
                    bits = list(seg[1:17])
                    self.huff[(seg[0] >> 4, seg[0] & 15)], seg = (bits, list(seg[17:17 + sum(bits)])), seg[17 + sum(bits):]
            elif m == 0xC0:
                assert seg[0] == 8
                self.H, self.W = seg[1] << 8 | seg[2], seg[3] << 8 | seg[4]
                self.comps = [[seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]] for i in range(seg[5])]
            elif m == 0xDD:
                self.ri = seg[0] << 8 | seg[1]
            elif m == 0xDA:
                assert seg[0] == len(self.comps)
                for i, c in enumerate(self.comps):
                    assert seg[1 + 2 * i] == c[0]
                    c += [seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15]
                pos += 2 + ln
                break
            else:
                assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xDC)
            pos += 2 + ln
        end = data.rfind(b"\xff\xd9")
        self.scan = data[pos:end if end >= pos else len(data)]
        self.hs, self.vs = (self.comps[0][1], self.comps[0][2]) if len(self.comps) == 3 else (1, 1)
        self.mcols, self.mrows = -(-self.W // (8 * self.hs)), -(-self.H // (8 * self.vs))
        # an MCU's blocks: (component, block row, block column) inside the MCU
        self.mcu = [(0, k // self.hs, k % self.hs) for k in range(self.hs * self.vs)] + [(1, 0, 0), (2, 0, 0)] if len(self.comps) == 3 else [(0, 0, 0)]
        self.nblocks = self.mcols * self.mrows * len(self.mcu)


def codes(bits, vals):
    """Annex C: (length, code) -> symbol"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def entropy(st):
    """the scan -> (nblocks, 64) int64 in scan order, natural coefficient order, the DC as the difference the stream holds.  The restart intervals are split at their
    markers, every interval is unstuffed and read bit by bit."""
    dct = [codes(*st.huff[(0, c[4])]) for c in st.comps]
    act = [codes(*st.huff[(1, c[5])]) for c in st.comps]
    out = np.zeros((st.nblocks, 64), np.int64)
    parts, start, i, scan = [], 0, 0, st.scan
    while True:      # cut at RSTm
        i = scan.find(b"\xff", i)
        if i < 0 or i + 1 >= len(scan):
            break
        if 0xD0 <= scan[i + 1] <= 0xD7:
            parts.append(scan[start:i])
            start = i + 2
        i += 2
    parts.append(scan[start:])
    blk = 0
    for part in parts:
        raw = part.replace(b"\xff\x00", b"\xff")
        acc, total, pos = int.from_bytes(raw, "big"), 8 * len(raw), 0

        def take(n):
            nonlocal pos
            assert pos + n <= total
            v = (acc >> (total - pos - n)) & ((1 << n) - 1)
            pos += n
            return v

        def symbol(table):
            code = 0
            for length in range(1, 17):
                code = code << 1 | take(1)
                if (length, code) in table:
                    return table[(length, code)]
            raise AssertionError("no such code")

        def value(size):
            v = take(size) if size else 0
            return v - (1 << size) + 1 if size and v < 1 << (size - 1) else v

        n_mcu = st.ri if st.ri else st.mcols * st.mrows
        for _ in range(n_mcu):
            if blk >= st.nblocks:
                break
            for comp, _, _ in st.mcu:
                zz = np.zeros(64, np.int64)
                zz[0] = value(symbol(dct[comp]))
                k = 1
                while k < 64:
                    s = symbol(act[comp])
                    run, size = s >> 4, s & 15
                    if size == 0:
                        if run != 15:
                            break
                        k += 16
                        continue
                    k += run
                    zz[k] = value(size)
                    k += 1
                out[blk, ZIG] = zz
                blk += 1
    assert blk == st.nblocks
    return out


def dc_values(st, diffs):
    """the DC differences -> values: a running sum per component in scan order, from 0 again after every restart interval"""
    out = diffs.copy()
    bpm = len(st.mcu)
    pred = [0, 0, 0]
    for b in range(st.nblocks):
        if st.ri and b % (st.ri * bpm) == 0:
            pred = [0, 0, 0]
        c = st.mcu[b % bpm][0]
        pred[c] += int(diffs[b, 0])
        out[b, 0] = pred[c]
    return out


def _idct_1d(d, shift):
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    z1 = (d2 + d6) * 4433
    t2, t3 = z1 + d6 * -15137, z1 + d2 * 6270
    t0, t1 = (d0 + d4) << 13, (d0 - d4) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = d7 + d1, d5 + d3, d7 + d3, d5 + d1
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = d7 * 2446, d5 * 16819, d3 * 25172, d1 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    rnd = 1 << (shift - 1)
    return np.stack([(v + rnd) >> shift for v in (e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3)], -1)


def idct(blocks):
    """(..., 8, 8) dequantised coefficients -> samples 0 .. 255: columns (descale 11), rows (descale 18), + 128, clip"""
    cols = np.swapaxes(_idct_1d(np.swapaxes(blocks, -1, -2), 11), -1, -2)
    return np.clip(_idct_1d(cols, 18) + 128, 0, 255)


def planes(st, coefs):
    """-> one plane per component, whole blocks (the padding included)"""
    bpm, out = len(st.mcu), []
    grid = coefs.reshape(st.mrows, st.mcols, bpm, 8, 8)
    for c, comp in enumerate(st.comps):
        ks = [k for k, m in enumerate(st.mcu) if m[0] == c]
        h, v = (st.hs, st.vs) if c == 0 else (1, 1)
        px = idct(grid[:, :, ks] * st.qt[comp[3]].reshape(8, 8))      # (mrows, mcols, v * h, 8, 8)
        px = px.reshape(st.mrows, st.mcols, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(st.mrows * v * 8, st.mcols * h * 8)
        out.append(px)
    return out


def upsample(st, p):
    """a chroma plane -> the luminance plane's size (at least): libjpeg's triangle filters over the component's real extent"""
    dh, dw = -(-st.H // st.vs), -(-st.W // st.hs)
    p = p[:dh, :dw]
    if st.hs == 1:
        return p
    if dw <= 2:
        return np.repeat(np.repeat(p, st.vs, 0), 2, 1)
    if st.vs == 2:
        up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
        s = np.empty((2 * dh, dw), np.int64)
        s[0::2], s[1::2] = 3 * p + up, 3 * p + dn
        r1, r2 = 8, 7
    else:
        s, r1, r2 = p, 1, 2
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * dw), np.int64)
    sh = 4 if st.vs == 2 else 2
    out[:, 0::2], out[:, 1::2] = (3 * s + left + r1) >> sh, (3 * s + right + r2) >> sh
    return out


def frame(st, coefs):
    """coefficients (DC values) -> (H, W, 3) uint8 BGR"""
    pl = planes(st, coefs)
    y = pl[0][:st.H, :st.W]
    if len(pl) == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    cb, cr = [upsample(st, p)[:st.H, :st.W] - 128 for p in pl[1:]]
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data, stages=False):
    """-> the frame; stages=True: (coefficients with DC differences, coefficients with DC values, frame)"""
    st = Stream(data)
    diffs = entropy(st)
    coefs = dc_values(st, diffs)
    out = frame(st, coefs)
    return (diffs, coefs, out) if stages else out


# ---- the self-synchronising scheme: a restatement that counts ----
def _unstuffed(scan):
    """the scan's data bytes with the stuffed index of each, cut at the first marker that is not RSTm; RSTm bytes are kept as markers (value -1 - m)"""
    vals, idx, i = [], [], 0
    while i < len(scan):
        c = scan[i]
        if c == 0xFF:
            nxt = scan[i + 1] if i + 1 < len(scan) else 0xD9
            if nxt == 0:
                vals.append(0xFF); idx.append(i); i += 2
                continue
            if 0xD0 <= nxt <= 0xD7:
                vals.append(-1); idx.append(i); i += 2
                continue
            break
        vals.append(c); idx.append(i); i += 1
    return vals, idx


def sync_rounds(data, subseq_bytes, lanes=256):
    """-> (launches that found work, most rounds inside a run, runs): every lane decodes the symbols that start inside its subsequence of stuffed bytes, first from
    the assumed state (its first bit, block 0, coefficient 0), then again whenever its predecessor's exit state differs from the state it entered with; a run of
    `lanes` lanes repeats that until nothing changes, and launch r > 0 re-enters the runs whose predecessor's exit changed in launch r - 1.  Only for streams
    WITHOUT restart markers (their treatment is the device's own affair), positions in unstuffed bits with the subsequence bounds mapped through the stuffing."""
    st = Stream(data)
    assert st.ri == 0
    vals, idx = _unstuffed(st.scan)
    acc, total = int.from_bytes(bytes(vals), "big"), 8 * len(vals)
    # a data byte's position: behind the data byte before it (so a stuffed zero belongs to the byte that follows it) -> the first data byte at or after a stuffed index
    stuffed_to_data = np.searchsorted(np.array([0] + [i + 1 for i in idx[:-1]]), np.arange(len(st.scan) + 1))
    dct = [codes(*st.huff[(0, c[4])]) for c in st.comps]
    act = [codes(*st.huff[(1, c[5])]) for c in st.comps]
    look = []
    for tables in (dct, act):
        per = []
        for t in tables:
            lut = {}
            for (length, code), sym in t.items():
                lut.setdefault(length, {})[code] = sym
            per.append(lut)
        look.append(per)
    bpm, comp_of = len(st.mcu), [m[0] for m in st.mcu]
    S = subseq_bytes
    nsub = -(-len(st.scan) // S)
    bound = [8 * int(stuffed_to_data[min(s * S, len(st.scan))]) for s in range(nsub + 1)]
    bound[-1] = total

    def lane(state, end):
        p, b, z = state
        while p < end:
            window = (acc >> max(total - p - 32, 0)) << max(p + 32 - total, 0) & 0xFFFFFFFF if p < total else 0
            lut, sym, length = look[0 if z == 0 else 1][comp_of[b]], 0, 16
            for L in range(1, 17):
                d = lut.get(L)
                if d is not None and (window >> (32 - L)) in d:
                    sym, length = d[window >> (32 - L)], L
                    break
            size = min(sym if z == 0 else sym & 15, 11)
            if p + length + size > total:
                return (total, 0, 0)
            if z == 0:
                z = 1
            elif sym & 15 == 0:
                z = z + 16 if sym >> 4 == 15 else 64
            else:
                z = min(z + (sym >> 4), 63) + 1
            if z >= 64:
                z, b = 0, (b + 1) % bpm
            p += length + size
        return (p, b, z)

    nruns = -(-nsub // lanes)
    entry, exit_ = [None] * nsub, [None] * nsub
    run_entry, run_exit, worked, most = [None] * nruns, [None] * nruns, 0, 0
    for r in range(nruns):
        prev, any_work = list(run_exit), False
        for g in range(nruns):
            e = (0, 0, 0) if g == 0 else ((bound[g * lanes], 0, 0) if r == 0 else prev[g - 1])
            if r > 0 and e == run_entry[g]:
                continue
            any_work = True
            s0, n = g * lanes, min(lanes, nsub - g * lanes)
            iters = 0
            while True:
                if iters == 0:
                    todo = [(t, e if t == 0 else (bound[s0 + t], 0, 0)) for t in range(n)] if r == 0 else [(0, e)]
                else:
                    todo = [(t, e if t == 0 else exit_[s0 + t - 1]) for t in range(n)]
                    todo = [(t, w) for t, w in todo if w != entry[s0 + t]]
                for t, w in todo:
                    entry[s0 + t] = w
                new = {t: lane(w, bound[s0 + t + 1]) for t, w in todo}
                for t, x in new.items():
                    exit_[s0 + t] = x
                iters += 1
                if not todo:
                    break
            run_entry[g], run_exit[g], most = e, exit_[s0 + n - 1], max(most, iters)
        if any_work:
            worked = r + 1
    return worked, most, nruns
