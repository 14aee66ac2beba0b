"""Reference for the Merkle-leaf validation tests: the oracle's `validate`
records, reduced per leaf in Python ints. A leaf holds the records with
left < token <= right; its hash is the XOR of their 32-byte hashes and an empty
leaf is 32 zero bytes."""
import struct

INT64_MIN = -(2 ** 63)
INT64_MAX = 2 ** 63 - 1
ZERO = bytes(32)


def read_records(path):
    """[(token, 32-byte hash)] of an oracle/gpuc validate file, in file order."""
    raw = open(path, "rb").read()
    assert len(raw) % 40 == 0, len(raw)
    return [(struct.unpack_from(">q", raw, o)[0], raw[o + 8:o + 40])
            for o in range(0, len(raw), 40)]


def leaf_ranges(trees):
    """Flat [(left_exclusive, right_inclusive)] of a tree list
    [(left_exclusive, [leaf_right, ...])]."""
    out = []
    for left, rights in trees:
        prev = left
        for r in rights:
            out.append((prev, r))
            prev = r
    return out


def reduce_leaves(records, trees, token_range=None):
    """(hashes, counts, n_partitions) the device reduction must give. Records
    come token-sorted and leaves ascend, so one forward walk over both places
    every record: no search, nothing shared with the library's lookup."""
    ranges = leaf_ranges(trees)
    acc = [0] * len(ranges)
    cnt = [0] * len(ranges)
    assert all(a[0] <= b[0] for a, b in zip(records, records[1:]))
    i = 0
    for tok, h in records:
        if token_range is not None and not token_range[0] <= tok <= token_range[1]:
            continue
        while i < len(ranges) and ranges[i][1] < tok:
            i += 1
        if i < len(ranges) and ranges[i][0] < tok <= ranges[i][1]:
            acc[i] ^= int.from_bytes(h, "big")
            cnt[i] += 1
    return [a.to_bytes(32, "big") for a in acc], cnt, sum(cnt)


def even_split(n_leaves, lo=INT64_MIN, hi=INT64_MAX):
    """One tree over (lo, hi] cut into n_leaves leaves with integer arithmetic."""
    span = hi - lo
    rights = [lo + span * (i + 1) // n_leaves for i in range(n_leaves)]
    assert rights[-1] == hi and all(a < b for a, b in zip(rights, rights[1:]))
    return [(lo, rights)]
