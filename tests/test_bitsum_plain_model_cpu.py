"""CPU suite: the PLAIN term layout of the multiplication-free bucket reduction (bazuka_amd/csrc/msm_impl.cuh section 6b, msm_bitsum_quad_kernel<128, true>), on
integers - the sibling of tests/test_bitsum_model_cpu.py, which does the same for the paired layout.

    sum_b (b + 1) B_b  =  S_tot + sum_k 2^k S_k,    S_k = sum of the buckets whose index has bit k set

A call that reduces exactly one bucket set (a full window table's) leaves c terms: S_k at index k (bit position k, k < c - 1) and the plain sum at index c - 1
(position 0).  One workgroup of 256 lanes per term runs ONE tree over 256 slots: lane t holds leaves t, t + 256, ... (two at most at c <= 21), the tree starts at
min(256, leaves) slots.  This file restates the lane -> leaf map, the term indices and the Horner's positions (msm_horner_terms_set with plain = true) over the
group Z, for c - 1 = 10 .. 20 - both parities, so lbits = hbits and lbits = hbits + 1.  The device code itself is pinned by tests/test_gpu_msm_table_terms.py."""
import numpy as np
import pytest

TREE = 256  # lanes, and LDS slots, of the workgroup's one tree


def split(cm1):
    lbits = (cm1 + 1) // 2
    return lbits, cm1 - lbits


def row_col_sums(b, lbits, hbits):
    """what msm_rowcol_quad_kernel leaves (its own lane maps: tests/test_bitsum_model_cpu.py): b = L h + l"""
    m = b.reshape(1 << hbits, 1 << lbits)
    return [int(x) for x in m.sum(axis=1)], [int(x) for x in m.sum(axis=0)]


def leaf_index(j, bit):
    return ((((j >> bit) << 1) | 1) << bit) | (j & ((1 << bit) - 1))


def plain_terms(rows, cols, lbits, hbits):
    """msm_bitsum_quad_kernel<128, true>: workgroup t < n_bits sums the sources with bit t set, workgroup n_bits every row sum"""
    n_bits = lbits + hbits
    out = []
    for t in range(n_bits + 1):
        total = t == n_bits
        from_cols = not total and t < lbits
        n_src = 1 << (lbits if from_cols else hbits)
        bit = 0 if total else (t if from_cols else t - lbits)
        src = cols if from_cols else rows
        n_leaves = n_src if total else n_src // 2
        sh, seen = [0] * TREE, []
        for tid in range(TREE):                       # a lane's serial walk: identities in the slots beyond the leaves
            for j in range(tid, n_leaves, TREE):
                i = j if total else leaf_index(j, bit)
                assert i < n_src and (total or (i >> bit) & 1)
                seen.append(i)
                sh[tid] += src[i]
        assert len(seen) == len(set(seen)) == n_leaves              # every leaf once
        assert max(len(range(tid, n_leaves, TREE)) for tid in range(TREE)) == max(1, n_leaves // TREE)
        levels_from = 1
        while levels_from < TREE and levels_from < n_leaves:
            levels_from <<= 1
        assert all(x == 0 for x in sh[levels_from:])                # nothing outside the tree's first level
        s = levels_from // 2
        while s > 0:
            for p in range(s):
                sh[p] += sh[p + s]
            s //= 2
        out.append(sh[0])
    return out


def horner_plain(t, c):
    """msm_horner_terms_host(T, 1, c, 0, plain = true)"""
    assert len(t) == c
    acc = 0
    for bit in range(c - 1, -1, -1):
        acc *= 2
        if bit < c - 1:
            acc += t[bit]
        if bit == 0:
            acc += t[c - 1]
    return acc


def bucket_sets(cm1):
    """int64 arrays: 2^20 buckets below 2^20 weigh less than 2^60 in all"""
    half, rng = 1 << cm1, np.random.default_rng(cm1)
    yield "random", np.where(rng.random(half) < 0.7, rng.integers(0, 1 << 20, half), 0).astype(np.int64)  # empty buckets are identities
    for name, at in (("bucket 0", 0), ("top bucket", half - 1)):
        b = np.zeros(half, dtype=np.int64)
        b[at] = 7
        yield name, b
    yield "all zero", np.zeros(half, dtype=np.int64)


@pytest.mark.parametrize("cm1", list(range(10, 21)))
def test_plain_terms_at_their_positions_give_the_weighted_bucket_sum(cm1):
    c = cm1 + 1
    lbits, hbits = split(cm1)
    assert lbits + hbits == cm1 and lbits - hbits == cm1 % 2
    idx = np.arange(1 << cm1, dtype=np.int64)
    for name, b in bucket_sets(cm1):
        rows, cols = row_col_sums(b, lbits, hbits)
        terms = plain_terms(rows, cols, lbits, hbits)
        assert len(terms) == c, name
        for k in range(cm1):                                        # S_k at index k
            assert terms[k] == int(b[((idx >> k) & 1) == 1].sum()), (name, k)
        assert terms[cm1] == int(b.sum()), name                     # the plain sum at index n_bits
        assert horner_plain(terms, c) == int(((idx + 1) * b).sum()), name


def test_leaves_per_lane_at_the_table_window():
    """c = 20 (lbits = 10, hbits = 9): a column bit has 512 leaves and the plain sum 512 row sums - two per lane, one serial addition; a row bit 256 - one per lane"""
    lbits, hbits = split(19)
    assert (lbits, hbits) == (10, 9)
    assert ((1 << lbits) // 2) // TREE == 2 and (1 << hbits) // TREE == 2 and ((1 << hbits) // 2) // TREE == 1
