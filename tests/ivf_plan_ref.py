"""numpy restatement of dir_ivf_plan (include/dir_engine.h), written from the definition: the probe tables of a scan by list
from probe [Q, nprobe] and list_off [nlist + 1], and the host bound of the grid index.py launches the scan with.

A slot (q, p) probes list probe[q][p]; a list outside [0, nlist) makes it EMPTY (length 0).  With the flat index
f = q * nprobe + p:
  col_off[q][p]    the lengths of the slots (q, p') with p' < p added up;
  the pair order   the slots by (list, f) ascending with an empty slot counted as list nlist - a stable sort by list;
  pair_q, pair_col q and col_off[q][p] of the slot at every place of that order;
  pair_off         the CSR of the order by list, [nlist + 1]: pair_off[nlist] = the slots that are not empty;
  item_off         the CSR of ceil(len_l / 256) * ceil(pairs_l / 32), [nlist + 1];
  counts           (item_off[nlist], reach), reach = the largest col_off + length over the slots, 0 without a slot."""
import numpy as np

TILE_ROWS, GROUP = 256, 32


def plan(probe, list_off):
    """-> dict of int32 arrays col_off [Q, nprobe], pair_off, pair_q, pair_col, item_off, counts [2]"""
    probe = np.asarray(probe, np.int64)
    list_off = np.asarray(list_off, np.int64)
    Q, nprobe = probe.shape
    nlist = len(list_off) - 1
    lens = np.diff(list_off)
    real = (probe >= 0) & (probe < nlist)
    slot_len = np.where(real, lens[np.where(real, probe, 0)], 0)
    col_off = np.cumsum(slot_len, axis=1) - slot_len
    key = np.where(real, probe, nlist).reshape(-1)
    order = np.array(sorted(range(Q * nprobe), key=lambda f: (key[f], f)), np.int64)
    pair_off = np.array([(key < l).sum() for l in range(nlist + 1)], np.int64)
    pair_q = order // max(nprobe, 1)
    pair_col = col_off.reshape(-1)[order]
    pairs = np.diff(pair_off)
    per_list = -(-lens // TILE_ROWS) * -(-pairs // GROUP)
    item_off = np.concatenate([[0], np.cumsum(per_list)])
    reach = int((col_off + slot_len).max()) if Q * nprobe else 0
    out = dict(col_off=col_off, pair_off=pair_off, pair_q=pair_q, pair_col=pair_col, item_off=item_off,
               counts=np.array([item_off[-1], reach]))
    return {k: v.astype(np.int32) for k, v in out.items()}


def plan_brute(probe, list_off):
    """The same tables by loops over the sentences of the definition, one entry at a time (the check of plan)."""
    Q, nprobe = len(probe), len(probe[0]) if len(probe) else 0
    nlist = len(list_off) - 1
    length = lambda l: int(list_off[l + 1]) - int(list_off[l]) if 0 <= l < nlist else 0
    col_off = [[sum(length(int(probe[q][pp])) for pp in range(p)) for p in range(nprobe)] for q in range(Q)]
    pair_off, pair_q, pair_col, item_off = [0], [], [], [0]
    for l in list(range(nlist)) + [None]:                     # None: the empty slots, after every list
        members = [(q, p) for q in range(Q) for p in range(nprobe)
                   if (int(probe[q][p]) == l if l is not None else not 0 <= int(probe[q][p]) < nlist)]
        pair_q += [q for q, _ in members]
        pair_col += [col_off[q][p] for q, p in members]
        if l is not None:
            pair_off.append(pair_off[-1] + len(members))
            tiles, groups = (length(l) + TILE_ROWS - 1) // TILE_ROWS, (len(members) + GROUP - 1) // GROUP
            item_off.append(item_off[-1] + tiles * groups)
    reach = max([col_off[q][p] + length(int(probe[q][p])) for q in range(Q) for p in range(nprobe)] + [0])
    out = dict(col_off=np.array(col_off).reshape(Q, nprobe), pair_off=pair_off, pair_q=pair_q, pair_col=pair_col,
               item_off=item_off, counts=[item_off[-1], reach])
    return {k: np.asarray(v, np.int32) for k, v in out.items()}


def plain_bound(lens, rows, nprobe):
    """rows * T(nprobe), T(m) = the ceil(len / 256) of the m longest lists added up.  It bounds item_off[nlist] whenever the
    lists of one query are distinct: list l, probed by n_l queries, takes tiles_l * ceil(n_l / 32) <= tiles_l * n_l
    workgroups, and the sum of tiles_l * n_l over the lists is the sum over the queries of the tiles of their lists - at
    most the nprobe largest for each."""
    tiles = np.sort(-(-np.asarray(lens, np.int64) // TILE_ROWS))
    return int(rows) * int(tiles[len(tiles) - nprobe:].sum())


def items_bound(lens, rows, nprobe):
    """The host bound of the grid index.py launches a chunk of `rows` queries at nprobe lists each with:
    floor((rows * T(nprobe) + 31 * T(min(nlist, rows * nprobe))) / 32).  ceil(n / 32) <= (n + 31) / 32 for n >= 1, the first
    term bounds the sum of tiles_l * n_l as in plain_bound, and the lists with n_l >= 1 are at most min(nlist, rows *
    nprobe), so their tiles add up to at most T of that many."""
    tiles = np.sort(-(-np.asarray(lens, np.int64) // TILE_ROWS))[::-1]
    m = min(len(tiles), int(rows) * nprobe)
    return (int(rows) * int(tiles[:nprobe].sum()) + 31 * int(tiles[:m].sum())) // 32
