"""Exact models of the pruned scan's plan, in plain numpy (nothing of crackling_amd is imported here).

planned_comparisons() is LAYOUT-FREE: it knows the rule that decides which sites a guide has to be compared with (comment
above group_units in issl_bin.hip, README "pruned scan") and nothing of buckets, groups, tiles or units.

unit_model() FOLLOWS THE DOCUMENTED LAYOUT ("Short units"; group_units in issl_bin.hip): a bucket of a slice
holds its sites ordered by the byte of the four positions behind the slice, a group is the run of one byte value, and a
group [s0, s1) is covered from s0 & ~31 on by full units of 2048 candidates and one last unit of 512, 1024 or 2048.  A pull
request that changes that layout must change this function with it; planned_comparisons() stays as it is.

Signatures are the packed 20-mers of the index: 2 bits per position, position p at bits 2p .. 2p + 1."""
import numpy as np

SEQ_LEN = 20
UNIT = 2048          # candidates of a full unit
LANE_GROUP = 32      # a unit starts on a multiple of this inside its bucket
SMALL_PAIRS = 512    # (guide, slice) pairs of a batch that the one-launch binning takes


def successor_tolerance(max_dist):
    """Mismatches a site may have in the four positions behind an exactly matching slice and still have to be compared."""
    if not 0 <= max_dist <= 5:
        raise ValueError("the pruned scan takes max_dist 0..5")
    return 0 if max_dist <= 2 else 1 if max_dist <= 4 else 2


def small_batch_limit(slice_width, max_dist):
    """Guides up to which a batch is binned in one launch, every placement a group of its own (0: never)."""
    return SMALL_PAIRS // (2 * SEQ_LEN // slice_width) if max_dist <= 4 else 0


def _codes(sigs):
    sigs = np.asarray(sigs, dtype=np.uint64)
    return np.stack([((sigs >> np.uint64(2 * p)) & np.uint64(3)).astype(np.int64) for p in range(SEQ_LEN)], axis=1)


def _slice_and_successor(codes, s, slice_width):
    """-> (value of slice s, byte of the four positions that follow it cyclically; the first of them in the low bits)."""
    per = slice_width // 2
    value = np.zeros(len(codes), dtype=np.int64)
    for j in range(per):
        value |= codes[:, s * per + j] << (2 * j)
    succ = np.zeros(len(codes), dtype=np.int64)
    for j in range(4):
        succ |= codes[:, (s * per + per + j) % SEQ_LEN] << (2 * j)
    return value, succ


def _near(k):
    """256 x 256: bytes of four positions that differ in at most k of them."""
    x = np.arange(256)[:, None] ^ np.arange(256)[None, :]
    diff = ((x | (x >> 1)) & 0x55)
    count = (diff & 1) + ((diff >> 2) & 1) + ((diff >> 4) & 1) + ((diff >> 6) & 1)
    return (count <= k).astype(np.float64)   # (products of counts below 2^31 with 0 / 1: exact in float64, and a BLAS call)


def site_tables(site_sigs, slice_width):
    """Per slice: sites by [value of the slice, byte behind it].  All that the two counts below need of the sites; either
    takes this list in place of the signatures, for an index that is asked about many batches."""
    if isinstance(site_sigs, list):
        return site_sigs
    sc = _codes(site_sigs)
    out = []
    for s in range(2 * SEQ_LEN // slice_width):
        sv, sb = _slice_and_successor(sc, s, slice_width)
        out.append(np.bincount(sv * 256 + sb, minlength=256 << slice_width).reshape(-1, 256))
    return out


def visits(site_sigs, guide_sigs, max_dist, slice_width, k=None):
    """Pairs (site_sigs[i], guide_sigs[i]) -> bool [n, n_slices]: the slices in whose bucket the guide has to meet the site."""
    k = successor_tolerance(max_dist) if k is None else k
    sc, gc = _codes(site_sigs), _codes(guide_sigs)
    per, out = slice_width // 2, []
    for s in range(SEQ_LEN // per):
        same = np.ones(len(sc), dtype=bool)
        for j in range(per):
            same &= sc[:, s * per + j] == gc[:, s * per + j]
        off = np.zeros(len(sc), dtype=np.int64)
        for j in range(4):
            p = (s * per + per + j) % SEQ_LEN
            off += sc[:, p] != gc[:, p]
        out.append(same & (off <= k))
    return np.stack(out, axis=1)


def planned_comparisons(site_sigs, guide_sigs, max_dist, slice_width, k=None):
    """Over every guide and every slice: the sites that agree with the guide on the slice and differ from it in at most k
    of the four positions behind the slice.  k from max_dist unless given (k = 4: the whole bucket)."""
    k = successor_tolerance(max_dist) if k is None else k
    tables, gc = site_tables(site_sigs, slice_width), _codes(guide_sigs)
    near, total = _near(k), 0
    for s, sites in enumerate(tables):
        gv, gb = _slice_and_successor(gc, s, slice_width)
        total += int(np.rint(sites.astype(np.float64) @ near).astype(np.int64)[gv, gb].sum())   # [slice value, byte]: the sites a guide of that value and byte counts
    return total


def group_units(s0, s1, blen, tail_shapes=1):
    """Units of the group [s0, s1) of a bucket of blen candidates (arrays or numbers).
    -> (units, candidates one guide is counted for over them, candidates per lane of the last unit: 8, 16 or 32 -- 32
    also where the span is a multiple of 2048 and the last unit is a full one)."""
    s0, s1, blen = (np.asarray(x, dtype=np.int64) for x in (s0, s1, blen))
    start = s0 - s0 % LANE_GROUP
    span = s1 - start
    n_full, rest = span // UNIT, span % UNIT
    shape = np.where((rest > 1024) | (rest == 0) | (tail_shapes == 0), 32, np.where(rest > 512, 16, 8))
    last_start = start + n_full * UNIT
    # (a full unit ends inside the group, so the bucket holds all 2048; only a last unit can reach past the bucket's end)
    last = np.where(rest > 0, np.minimum(blen - last_start, 64 * shape), 0)
    return n_full + (rest > 0), n_full * UNIT + last, shape


def unit_model(site_sigs, guide_sigs, max_dist, slice_width, item_guides=512, tail_shapes=1, small_batch=False):
    """-> (scan_tiles, candidates) of issl_stats after a pruned call.  small_batch: the batch has at most
    small_batch_limit() guides (and max_dist <= 4), so every placement of a guide is a group with one guide in it."""
    k = successor_tolerance(max_dist)
    if max_dist == 5:
        tail_shapes = 0   # three classes of guides: full shapes only
    tables, gc = site_tables(site_sigs, slice_width), _codes(guide_sigs)
    near, tiles, cands = _near(k), 0, 0
    for s, sites in enumerate(tables):
        gv, gb = _slice_and_successor(gc, s, slice_width)
        guides = np.bincount(gv * 256 + gb, minlength=256 << slice_width).reshape(-1, 256).astype(np.float64) @ near
        guides = np.rint(guides).astype(np.int64)
        s1 = np.cumsum(sites, axis=1)                      # groups in the order of the byte, inside their bucket
        s0, blen = s1 - sites, np.broadcast_to(s1[:, -1:], sites.shape)
        use = (sites > 0) & (guides > 0)                   # a group without candidates takes no guides
        units, counted, _ = group_units(s0[use], s1[use], blen[use], tail_shapes)
        c = guides[use]
        tiles += int((units * (c if small_batch else -(-c // item_guides))).sum())
        cands += int((counted * c).sum())
    return tiles, cands
