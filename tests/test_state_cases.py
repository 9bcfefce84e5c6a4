"""Census of tests/statecases.py's two-act traces, from the oracle alone: the
continuation tests of tests/test_state_gpu.py can only fail with a loader that
drops the LRU order among equal stamps or the free list's order if act 2
expires entries of act 1 that share a stamp and allocates from what act 1
freed. These are conditions on the traces; the seeds in statecases.SEEDS are
chosen so that the oracle meets them. CPU only."""
import numpy as np
import pytest

import statecases as SC


@pytest.fixture(scope="module")
def counted():
    return {}


def _census(counted, kind, variant):
    if (kind, variant) not in counted:
        counted[kind, variant] = SC.census(kind, variant)
    return counted[kind, variant]


@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_census(counted, kind, variant):
    c = _census(counted, kind, variant)
    live, ts = c["live_at_cut"], c["ts_at_cut"]
    exp = c["expired"]
    stamps, cnt = np.unique(ts[exp], return_counts=True)
    tied = int(cnt[cnt > 1].sum())
    born = c["born"]
    free_at_cut = ~live
    on_stack = free_at_cut & c["used"]
    never = free_at_cut & ~c["used"]
    fig = dict(live_at_cut=int(live.sum()), expired_in_act1=c["expired_in_act1"],
               expire_after_cut=int(exp.sum()), tied=tied, born=int(born.sum()),
               born_on_freed=int((born & c["freed_before"]).sum()),
               born_on_stack=int((born & on_stack).sum()),
               born_on_never_used=int((born & never).sum()))
    print(kind, variant, fig)
    # act 1 allocates, expires and allocates again
    assert fig["expired_in_act1"] >= 32
    assert fig["expire_after_cut"] >= 32
    assert fig["tied"] >= 8
    assert fig["born"] >= 32
    assert fig["born_on_freed"] >= 8
    if variant == "part":
        assert int(on_stack.sum()) >= 8 and int(never.sum()) >= 8
        assert fig["born_on_stack"] >= 8
        assert fig["born_on_never_used"] >= 8
    else:
        assert fig["live_at_cut"] == SC.CAP


@pytest.mark.parametrize("variant", SC.VARIANTS)
def test_vignat_new_flows_carry_many_external_ports(counted, variant):
    """Act 2's frames of flows that opened after the cut leave on the WAN
    device with the external port start_port + index (start_port 0) as their
    source port."""
    c = _census(counted, "nat", variant)
    (_, _, dv, _), cut = SC.trace("nat", variant)
    out, fr = c["out"], c["frames"]
    sent = np.nonzero((np.arange(out.shape[0]) >= cut) & (dv == 0) & (out == 1))[0]
    ports = fr[sent, 34].astype(int) | (fr[sent, 35].astype(int) << 8)  # (raw u16, as the NAT stores it)
    new_ports = set(int(p) for p in ports if p < SC.CAP and c["born"][p])
    print("nat", variant, "external ports of new flows:", len(new_ports))
    assert len(new_ports) >= 16
