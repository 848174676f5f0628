"""A CPU restatement of the bookkeeping of k_jpeg_frame's stages 1-5 (chalkydri_amd/csrc/k_jpeg.hip): the restart
intervals of a scan, their ends under the cap of MAX_BLOCK_BYTES per needed block, the pieces of CK_JPEG_SUB_BITS bits, the speculative
decode of every piece from "slot 0, DC next", the synchronisation rounds with their old and new exits, the ordered walk with its
early stop, and the completed-block count and block index of every piece.  No coefficients, no pixels: the model says which way
through the kernel a stream takes, never whether the device decoded it right (tests/np_jpeg.py and Pillow say that).
The constants are read from the sources, so a retune moves the cases' conditions instead of silently emptying them."""
import os
import re

import numpy as np

import np_jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chalkydri_amd", "csrc")


def constants(csrc=CSRC):
    def find(name, pattern):
        with open(os.path.join(csrc, name)) as f:
            m = re.search(pattern, f.read())
        assert m, (name, pattern)
        return int(m.group(1))
    return {"SUB_BITS": find("ck_jpeg.h", r"constexpr\s+int\s+CK_JPEG_SUB_BITS\s*=\s*(\d+)\s*;"),
            "FRAME_THREADS": find("ck_jpeg.h", r"constexpr\s+int\s+CK_JPEG_FRAME_THREADS\s*=\s*(\d+)\s*;"),
            "SYNC_ROUNDS": find("k_jpeg.hip", r"constexpr\s+int\s+SYNC_ROUNDS\s*=\s*(\d+)\s*;"),
            "MAX_BLOCK_BYTES": find("k_jpeg.hip", r"constexpr\s+uint32_t\s+MAX_BLOCK_BYTES\s*=\s*(\d+)\s*;")}


_luts = {}


def _lut(table):
    key = (tuple(table[0]), tuple(table[1]))
    if key not in _luts:
        _luts[key] = J._lut16(*table)
    return _luts[key]


class Trace:
    """What the exact chain of one interval met, counted over its first `need` blocks (tail_*: after them)."""

    def __init__(self, base, sub, need):
        self.base, self.sub, self.need = base, sub, need
        self.blocks = []          # (first bit, bit after the last) of every completed block
        self.mcu_starts = []      # first bit of every block that opens an MCU
        self.max_zrl = self.no_eob_blocks = self.long_codes = self.codes16 = self.eob_run_syms = 0
        self.code_straddles = self.field_straddles = self.tail_invalid = self.tail_runpast = 0

    def span(self, p0, p1, what):   # bits [p0, p1) of one code or one value field
        if p1 > p0 and len(self.blocks) < self.need and (p0 - self.base) // self.sub != (p1 - 1 - self.base) // self.sub:
            setattr(self, what, getattr(self, what) + 1)


def decode_run(win, far, luts, bpm, nyb, pos, slot, zz, end, lim, tr=None):
    """decode_run<false> of k_jpeg.hip: every code that starts before `end`, from the state (pos, slot, zz); an invalid code
    resumes one bit on at a block start, a run past 63 at a block start.  -> (pos, slot, zz, blocks completed at or before lim)"""
    nb = 0
    zrl, start = 0, pos
    while pos < end:
        dcl, acl = luts[0 if slot < nyb else slot - nyb + 1]
        w = 0xFFFF if pos >= far else ((win[pos >> 3] << (pos & 7)) & 0xFFFFFFFF) >> 16
        e = (acl if zz else dcl)[w]
        if not e:
            if tr is not None and len(tr.blocks) >= tr.need:
                tr.tail_invalid += 1
            pos += 1
            zz = 0
            continue
        ln, sym = e >> 8, e & 255
        if tr is not None:
            if zz == 0:
                start, zrl = pos, 0
                if slot == 0:
                    tr.mcu_starts.append(pos)
            tr.span(pos, pos + ln, "code_straddles")
            if len(tr.blocks) < tr.need:
                tr.long_codes += ln > 9
                tr.codes16 += ln == 16
        pos += ln
        if zz == 0:
            if tr is not None:
                tr.span(pos, pos + sym, "field_straddles")
            pos += sym
            zz = 1
        else:
            rr, s = sym >> 4, sym & 15
            if s:
                zz += rr
                if zz > 63:
                    if tr is not None and len(tr.blocks) >= tr.need:
                        tr.tail_runpast += 1
                    zz = 0
                    continue
                if tr is not None:
                    tr.span(pos, pos + s, "field_straddles")
                pos += s
                zz += 1
                if tr is not None and zz >= 64 and len(tr.blocks) < tr.need:
                    tr.no_eob_blocks += 1
            elif rr == 15:
                if zz + 15 > 63:
                    if tr is not None and len(tr.blocks) >= tr.need:
                        tr.tail_runpast += 1
                    zz = 0
                    continue
                zz += 16
                zrl += 1
            else:
                if tr is not None and rr and len(tr.blocks) < tr.need:
                    tr.eob_run_syms += 1
                zz = 64
        if zz >= 64:
            if pos <= lim:
                nb += 1
                if tr is not None:
                    if len(tr.blocks) < tr.need:
                        tr.max_zrl = max(tr.max_zrl, zrl)
                    tr.blocks.append((start, pos))
            zz = 0
            slot = 0 if slot + 1 == bpm else slot + 1
    return pos, slot, zz, nb


def run(data, consts=None, early_stop=True):
    """The model's figures for one stream (a dict); {"refused": status} for a stream the host or the unstuffer refuses.
    early_stop=False takes the walk's `done_blocks < need` stop out (the liveness check of the stale-piece readout)."""
    K = consts or constants()
    SUB, ROUNDS, MAXB = K["SUB_BITS"], K["SYNC_ROUNDS"], K["MAX_BLOCK_BYTES"]
    try:
        P = J.parse(data)
    except J.JpegError as e:
        return {"refused": J.UNSUPPORTED if e.code == "EUNSUPPORTED" else J.CORRUPT}
    w, h, nc = P["width"], P["height"], P["n_components"]
    H, V = (P["h_samp"], P["v_samp"]) if nc == 3 else (1, 1)
    nyb = H * V
    bpm = nyb + 2 if nc == 3 else 1
    nmcu = -(-w // (8 * H)) * -(-h // (8 * V))
    R = P["restart_interval"] or nmcu
    nint = -(-nmcu // R)
    comp, rst = J.unstuff(bytes(data)[P["scan_off"]:])
    if len(rst) != nint - 1 or any(r != (k & 7) for k, (_, r) in enumerate(rst)):
        return {"refused": J.CORRUPT}
    starts = [0] + [o for o, _ in rst] + [len(comp)]
    c = np.frombuffer(comp + b"\xff" * 8, np.uint8).astype(np.int64)
    win = ((c[:-3] << 24) | (c[1:-2] << 16) | (c[2:-1] << 8) | c[3:]).tolist()
    far = len(comp) * 8 + 32
    luts = [(_lut(dct), _lut(act)) for dct, act in P["tables"]]

    # ---- 2. intervals and pieces ----------------------------------------------------------------------------------------------
    need, lim, first, p_start, p_end, p_int, cap_cut = [], [], [], [], [], [], 0
    for k in range(nint):
        n = min(R, nmcu - k * R) * bpm
        b0, b1 = starts[k], min(starts[k + 1], starts[k] + MAXB * n)
        cap_cut += b1 < starts[k + 1]
        need.append(n)
        lim.append(b1 * 8)
        first.append(len(p_start))
        for j in range(max(1, -(-(b1 - b0) * 8 // SUB))):
            p_start.append(b0 * 8 + j * SUB)
            p_end.append(min(b0 * 8 + (j + 1) * SUB, b1 * 8))
            p_int.append(k)
    npieces = len(p_start)
    is_first = [False] * npieces
    for s in first:
        is_first[s] = True
    memo = {}

    def decode(s, state):
        if (s, state) not in memo:
            memo[(s, state)] = decode_run(win, far, luts, bpm, nyb, state[0], state[1], state[2], p_end[s], lim[p_int[s]])
        r = memo[(s, state)]
        return r[:3], r[3]

    # ---- 3. speculative decode ----------------------------------------------------------------------------------------------------
    entry = [(p_start[s], 0, 0) for s in range(npieces)]
    exit_, nb = [None] * npieces, [0] * npieces
    for s in range(npieces):
        exit_[s], nb[s] = decode(s, entry[s])
    # ---- 4. rounds (old and new exits), to the end; the state after SYNC_ROUNDS of them is the kernel's -------------------------
    rounds = [0] * nint
    snapshot, n_round = None, 0
    while True:
        if n_round == ROUNDS:
            snapshot = (list(entry), list(exit_), list(nb))
        new_exit, changed = list(exit_), set()
        for s in range(npieces):
            if not is_first[s] and exit_[s - 1] != entry[s]:
                entry[s] = exit_[s - 1]
                new_exit[s], nb[s] = decode(s, entry[s])
                changed.add(p_int[s])
        if not changed:
            break
        exit_ = new_exit
        n_round += 1
        for k in changed:
            rounds[k] += 1
    frame_rounds = max(rounds)
    settled = frame_rounds < ROUNDS
    redecoded = stale = skipped = 0
    if not settled:
        entry, exit_, nb = snapshot
        for k in range(nint):
            s = first[k]
            prev, done = exit_[s], nb[s]
            j = s + 1
            while j < npieces and not is_first[j] and (done < need[k] or not early_stop):
                if entry[j] != prev:
                    entry[j] = prev
                    exit_[j], nb[j] = decode(j, prev)
                    redecoded += 1
                prev = exit_[j]
                done += nb[j]
                j += 1
            while j < npieces and not is_first[j]:
                skipped += 1
                stale += entry[j] != exit_[j - 1]
                j += 1
    # ---- 5. block index of every piece; the exact chain of every interval, traced -------------------------------------------------
    blk0, total = [0] * npieces, [0] * nint
    for s in range(npieces):
        blk0[s] = 0 if is_first[s] else blk0[s - 1] + nb[s - 1]
        total[p_int[s]] = blk0[s] + nb[s]
    fig = {"pieces": npieces, "intervals": nint, "rounds": rounds, "frame_rounds": frame_rounds, "path": "settled" if settled else "walk",
           "walk_redecoded": redecoded, "walk_stale": stale, "walk_skipped": skipped, "cap_cut": cap_cut,
           "short_intervals": sum(total[k] < need[k] for k in range(nint)), "need": need,
           "interval_bytes": [starts[k + 1] - starts[k] for k in range(nint)], "interval_start": starts[:-1],
           "last_piece": [(first[k + 1] if k + 1 < nint else npieces) - 1 for k in range(nint)], "first_piece": first,
           "dc_index": [k * R * nyb for k in range(nint)], "unstuffed_bytes": len(comp),
           "zero_block_pieces": sum(1 for s in range(npieces) if nb[s] == 0 and p_end[s] > p_start[s] and blk0[s] < need[p_int[s]]),
           "blocks": [], "end_bits": [], "first_block_end": [], "spanning_blocks": 0, "mcu_aligned_pieces": 0, "max_zrl": 0}
    sums = ("no_eob_blocks", "long_codes", "codes16", "eob_run_syms", "code_straddles", "field_straddles", "tail_invalid", "tail_runpast")
    for name in sums:
        fig[name] = 0
    for k in range(nint):
        tr = Trace(starts[k] * 8, SUB, need[k])
        decode_run(win, far, luts, bpm, nyb, starts[k] * 8, 0, 0, lim[k], lim[k], tr)
        if not stale:
            assert len(tr.blocks) == total[k], ("the synchronised pieces do not add up to the exact chain", k, len(tr.blocks), total[k])
        fig["blocks"].append(min(len(tr.blocks), need[k]))
        fig["end_bits"].append(tr.blocks[need[k] - 1][1] if len(tr.blocks) >= need[k] else None)
        fig["first_block_end"].append(tr.blocks[0][1] if tr.blocks else None)
        fig["spanning_blocks"] += sum(1 for a, b in tr.blocks[:need[k]] if (b - 1 - tr.base) // SUB - (a - tr.base) // SUB >= 2)
        bounds = set(p_start[first[k] + 1:fig["last_piece"][k] + 1])
        fig["mcu_aligned_pieces"] += len(bounds & set(tr.mcu_starts))
        fig["max_zrl"] = max(fig["max_zrl"], tr.max_zrl)
        for name in sums:
            fig[name] += getattr(tr, name)
    return fig
