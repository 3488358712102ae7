"""The context's grow-only workspace slab under a sequence of different calls: every call lays its temporaries out afresh (bzk_ws.h WsLayout), the
slab moves when it grows and is re-used when it is large enough, and no call may see a stale pointer or another call's layout."""
import pytest

import decompress_cases as D
import eddsa_cases as E
import withdraw_cases as Wd
from util import rand_scalars_bytes

pytestmark = pytest.mark.gpu


def test_one_context_through_growing_and_reused_slabs_equals_fresh_contexts(co):
    """signatures (600 B of workspace), an arity-7 Poseidon batch (1 MiB), a 2^10-point G1 MSM, five transactions, five withdrawals, then the first
    call again, all on ONE context: each output equals the same call's on a context of its own.  Every call returns BZK_OK (the binding raises
    otherwise), so the live-layout guard does not fire on any of these paths; the released size shows that the slab did grow on the way."""
    from bazuka_amd import Bzk
    pub, msg, sig = E.bulk(3, 77)
    rows = rand_scalars_bytes(4096 * 7, 70)
    bases, sc = co.g1_bases(61, 0, 1 << 10, nthreads=co.ncpu()), rand_scalars_bytes(1 << 10, 71)
    txs = [c[1] for c in D.tx_list()[:5]]
    tx_blob = b"".join(D.enc_tx(t) for t in txs)
    wd_blob = b"".join(Wd.enc(c[1]) for c in Wd.fixed_list()[:5])
    calls = [
        ("jubjub_verify_batch", lambda ctx: ctx.jubjub_verify_batch(pub, msg, sig)),
        ("poseidon_batch", lambda ctx: ctx.poseidon_batch(rows, 7)),
        ("msm_g1", lambda ctx: ctx.msm_g1(bases, sc)),
        ("mpn_tx_verify_batch", lambda ctx: ctx.mpn_tx_verify_batch(tx_blob, 5)),
        ("mpn_withdraw_verify_batch", lambda ctx: ctx.mpn_withdraw_verify_batch(wd_blob, 5)),
        ("jubjub_verify_batch again", lambda ctx: ctx.jubjub_verify_batch(pub, msg, sig)),
    ]
    want = []
    for name, call in calls:
        fresh = Bzk(0)
        try:
            want.append(call(fresh))
        finally:
            fresh.close()
    assert want[0] == bytes([1, 0, 1]) and want[5] == want[0]  # E.bulk: the even entries are valid, the odd ones are not
    assert want[2] == co.msm_g1(bases, sc, nthreads=co.ncpu())
    one = Bzk(0)
    try:
        for (name, call), w in zip(calls, want):
            assert call(one) == w, name
        assert one.trim() >= 4096 * 8 * 32  # at least the Poseidon batch's rows and hashes: the slab grew past the first call's
        assert calls[0][1](one) == want[0]  # and a trimmed context starts over
    finally:
        one.close()
