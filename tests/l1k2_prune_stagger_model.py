"""An event model of the half-step protocol of l1k2_prune_wide_kernel (l1k2_prune.hip): 8 waves, two barriers per
tile, waves 4-7 (the trailing group) half a tile behind waves 0-3 (the leading group).  Each wave is a generator
that mirrors the kernel's control flow and yields what the protocol is about: barriers, loads into the two
double-buffered LDS arrays ("F": the feature tile, "R": the raw rows), the wave's wait for its loads, reads of a
buffer, reads and raises of the bail flags, and the tiles it counts into the statistics.  `simulate` runs the waves
half-step by half-step (a half-step ends when every wave stands at a barrier), and `check` holds the record to the
rules:

  * every wave passes the same number of barriers (a wave that ends while others wait is a hang);
  * a read of buffer slot b for tile t finds tile t there from every wave, each load waited for by its issuer in an
    earlier half-step (so a wait and a barrier lie between the load and the read);
  * no load into a slot is issued in a half-step in which, or before which, some wave still reads the tile it replaces;
  * a flag is never read in the half-step in which it is raised.

PROTOCOL is what the kernel does; the other settings move one thing and must be caught."""
import collections

WAVES = 8
LEAD = WAVES // 2

# lead_raw: where a leading wave issues the raw rows of tile t + 1 ("C": top of C(t), the kernel; "M": top of M(t), a
# half-step early).  lead_feat: its features ("M": top of M(t), the kernel; "C-1": top of C(t - 1), a half-step early).
Protocol = collections.namedtuple("Protocol", "trail_first_barrier lead_raw lead_feat wait_before_mid")
PROTOCOL = Protocol(True, "C", "M", True)

Result = collections.namedtuple("Result", "barriers counted gave_up events problems")


def _wave(w, ntiles, raises, proto):
    """The kernel's loop for wave w.  raises(w, tile) -> bool: whether the share rule fires for it at that tile."""
    trail = w >= LEAD
    if ntiles > 0:
        yield ("issue", "F", 0)
        yield ("issue", "R", 0)
        yield ("wait",)
    yield ("barrier",)                      # the prologue's; not one of the 2n + 1
    if trail and proto.trail_first_barrier:
        yield ("barrier",)                  # B_0
    bailed = False
    tl = 0
    while tl < ntiles:
        has_next = tl + 1 < ntiles
        yield ("read", "F", tl)             # M(tl): the A operand
        if has_next:
            if trail or proto.lead_feat == "M" or tl == 0:
                yield ("issue", "F", tl + 1)
            if trail or proto.lead_raw == "M":
                yield ("issue", "R", tl + 1)
        if bailed:                          # a trailing wave, at the top of the tile after the flag's
            break
        if proto.wait_before_mid:
            yield ("wait",)
        yield ("barrier",)                  # mid-tile
        if not trail:
            bailed = yield ("flag", (tl + 1) & 1)
            if has_next and proto.lead_raw == "C":
                yield ("issue", "R", tl + 1)
            if tl + 2 < ntiles and proto.lead_feat == "C-1":
                yield ("issue", "F", tl + 2)
        if bailed:                          # a leading wave drops the tile whose M it has run
            break
        yield ("read", "R", tl)             # C(tl): the drains
        yield ("count", tl)
        if raises(w, tl):
            yield ("raise", tl & 1)
        yield ("barrier",)                  # end of tile
        if trail:
            bailed = yield ("flag", tl & 1)
        tl += 1
    if not trail and not bailed:
        yield ("barrier",)                  # B_2n
        bailed = yield ("flag", (tl + 1) & 1)
    yield ("end", bool(bailed))


def simulate(ntiles, raises=lambda w, tl: False, proto=PROTOCOL):
    gens = [_wave(w, ntiles, raises, proto) for w in range(WAVES)]
    flags = [False, False]
    barriers = [0] * WAVES
    counted = [[] for _ in range(WAVES)]
    gave_up = [None] * WAVES
    events, problems = [], []              # events: (half-step, wave, kind, ...); half-step -1 is the prologue
    half = -1
    while any(v is None for v in gave_up):
        snapshot, raised, flag_reads = list(flags), [], []
        arrived = 0
        for w, g in enumerate(gens):
            if gave_up[w] is not None:
                continue
            send = None
            while True:
                ev = g.send(send)
                send = None
                if ev[0] == "barrier":
                    arrived += 1
                    barriers[w] += half >= 0
                    break
                if ev[0] == "end":
                    gave_up[w] = ev[1]
                    break
                if ev[0] == "flag":
                    send = snapshot[ev[1]]
                    flag_reads.append(ev[1])
                elif ev[0] == "raise":
                    raised.append(ev[1])
                elif ev[0] == "count":
                    counted[w].append(ev[1])
                events.append((half, w) + ev)
        for slot in raised:
            if slot in flag_reads:
                problems.append("half-step %d: flag %d is read while it is raised" % (half, slot))
            flags[slot] = True
        ended = sum(v is not None for v in gave_up)
        if arrived and ended:
            problems.append("half-step %d: hang, %d waves wait at a barrier that %d ended waves never reach" % (half, arrived, ended))
            break
        half += 1
    return Result(barriers, counted, gave_up, events, problems)


def check(res):
    """The problems of a run: those found while it ran and what the record of loads, waits and reads shows."""
    problems = list(res.problems)
    if len(set(res.barriers)) != 1:
        problems.append("barrier counts differ: %r" % (res.barriers,))
    if len({tuple(c) for c in res.counted}) != 1:
        problems.append("waves counted different tiles: %r" % (res.counted,))
    if len(set(res.gave_up)) != 1:
        problems.append("waves disagree about leaving: %r" % (res.gave_up,))
    loads = collections.defaultdict(list)   # (buffer, slot, wave) -> [tile, half-step issued, half-step waited for or None]
    reads = []
    for ev in res.events:
        half, w, kind = ev[:3]
        if kind == "issue":
            loads[(ev[3], ev[4] & 1, w)].append([ev[4], half, None])
        elif kind == "wait":
            for key, ls in loads.items():
                if key[2] == w:
                    for l in ls:
                        if l[2] is None:
                            l[2] = half
        elif kind == "read":
            reads.append((half, w, ev[3], ev[4]))
            for iw in range(WAVES):
                ls = loads[(ev[3], ev[4] & 1, iw)]
                if not ls or ls[-1][0] != ev[4]:
                    problems.append("half-step %d: wave %d reads %s tile %d, wave %d's part of the slot holds %r" % (
                        half, w, ev[3], ev[4], iw, ls[-1][0] if ls else None))
                elif ls[-1][2] is None or ls[-1][2] >= half:
                    problems.append("half-step %d: wave %d reads %s tile %d, wave %d's load was waited for in %r" % (
                        half, w, ev[3], ev[4], iw, ls[-1][2]))
    for (buf, slot, iw), ls in loads.items():
        for tile, issued, _ in ls:
            late = [(h, w) for h, w, b, t in reads if b == buf and t == tile - 2 and h >= issued]
            if late:
                problems.append("%s tile %d is issued by wave %d in half-step %d; tile %d is still read there in %r" % (
                    buf, tile, iw, issued, tile - 2, late[:4]))
    return problems


def share_rule(surv_of, share, inherited=False, share_unit=1024, tile_pairs=64 * 64):
    """raises(w, tl) of the kernel's share rule for per-tile survivor counts surv_of(w, tl): the running share of
    tests/l1k2_prune_wide_model.py, kept per wave.  Tiles must be asked for in order, once each."""
    warm, skip = (4, 0) if inherited else (128, 2)
    recent = [0] * WAVES

    def raises(w, tl):
        s = surv_of(w, tl)
        recent[w] = 8 * s if tl <= skip else recent[w] + s - (recent[w] >> 3)
        limit = share if tl >= warm else max(share, share_unit * 3 // 4) if tl > skip else share_unit
        return recent[w] * (share_unit // 8) > limit * tile_pairs
    return raises
