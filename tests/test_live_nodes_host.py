"""CPU: the bookkeeping that gives every live training node of a module a workspace of its own (``sir_amd.leases``), driven
with stand-in buffers -- no torch tensor, no device.  ``test_live_nodes_gpu.py`` runs the programs this protects."""
import gc

import pytest

from sir_amd import leases


class Slot:
    """Stand-in for ``ops.Workspace``."""
    made = 0

    def __init__(self):
        Slot.made += 1


class Owner:
    """Stand-in for a node's ``ctx``: the lease's only strong reference."""

    def __init__(self, lease):
        self.lease = lease


@pytest.fixture
def pool():
    Slot.made = 0
    return leases.LeasePool(Slot(), Slot)


def test_take_and_release_keep_the_primary(pool):
    for _ in range(4):                               # the ordinary loop: forward, backward, forward, backward
        a = pool.take()
        assert a.slot is pool.primary and not a.shared and not a.released and pool.primary_held
        a.release()
        assert a.released and not pool.primary_held and not a.moved_on()
        a.release()                                  # a second backward through a retained graph releases again: no effect
        assert not pool.primary_held and not pool.free and len(pool.live) == 0
    assert Slot.made == 1                            # no spare was ever made


def test_take_while_taken_gives_a_different_buffer(pool):
    a = pool.take()
    b = pool.take()
    c = pool.take()
    assert a.slot is pool.primary and len({id(a.slot), id(b.slot), id(c.slot)}) == 3
    assert a.shared and b.shared and c.shared        # every node that overlapped another clones its gradients
    for lease in (a, b, c):
        lease.check()                                # held: nothing moved on
        lease.release()
    assert not pool.free and not pool.primary_held   # spares are dropped once nobody is live
    d = pool.take()
    assert d.slot is pool.primary and not d.shared   # the lone node after them is lone again


def test_release_out_of_order_and_reuse_of_a_spare(pool):
    a, b = pool.take(), pool.take()
    a.release()                                      # the first node's backward ran first
    assert not pool.primary_held and pool.live and not pool.free
    c = pool.take()
    assert c.slot is pool.primary and c.shared and b.shared
    b.release()
    assert pool.free == [b.slot]                     # kept while c is live
    d = pool.take()
    assert d.slot is b.slot and Slot.made == 2       # reused, not a third buffer
    d.release()
    c.release()
    assert not pool.free and not pool.primary_held and len(pool.live) == 0


def test_release_by_collection_of_an_owner_that_never_ran_backward(pool):
    owner = Owner(pool.take())
    other = pool.take()
    assert other.slot is not pool.primary
    del owner                                        # the graph was dropped: ctx collected, the lease with it
    gc.collect()
    assert not pool.primary_held and len(pool.live) == 1
    nxt = pool.take()
    assert nxt.slot is pool.primary
    other.release()
    nxt.release()
    assert not pool.free


def test_second_backward_after_the_buffer_moved_on_is_detected(pool):
    a = pool.take()
    a.check()
    a.release()
    a.check()                                        # backward again with no forward in between: the buffer is as it was
    b = pool.take()                                  # another forward took the same buffer
    assert b.slot is a.slot and a.moved_on()
    with pytest.raises(RuntimeError, match="retain_graph.*backward again after another forward on this model"):
        a.check()
    b.release()
    with pytest.raises(RuntimeError, match="retain_graph"):
        a.check()                                    # still gone after the other node finished
    b.check()
    # a spare that was dropped and never handed out again keeps what its node left
    c, d = pool.take(), pool.take()
    d.release()
    c.release()
    d.check()


def test_train_state_carries_one_pool_over_the_module_primary():
    """``train_ops`` builds the pool over the module's own workspace (``_sir_train["ws"]``, which the suite's helpers read) and
    keeps it when the gradient buffer is rebuilt for a new weight token."""
    import torch
    from sir_amd import ops, train_ops
    from sir_amd.models.models import CNNAudioGRU
    m = CNNAudioGRU(5)
    st = train_ops._train_state(m)
    assert isinstance(st["pool"], leases.LeasePool) and st["pool"].primary is st["ws"] and isinstance(st["ws"], ops.Workspace)
    lease = st["pool"].take()
    m._sir_token = ops.new_model_token()             # (what load_state_dict / a replaced tensor does)
    st2 = train_ops._train_state(m)
    assert st2 is not st and st2["pool"] is st["pool"] and st2["ws"] is st["ws"] and st2["pool"].primary_held
    lease.release()
    # the stamp a node records: the parameters' version counters and the parameter writes torch does not count
    s0 = train_ops._input_stamp(m)
    assert train_ops._input_stamp(m) == s0
    with torch.no_grad():
        m.fc.bias.add_(1.0)
    s1 = train_ops._input_stamp(m)
    assert s1 != s0
    ops.bump_weights_epoch()                         # FusedAdam.step, weights_changed, broadcast_module_
    s2 = train_ops._input_stamp(m)
    assert s2 != s1
    epoch = ops._weights_epoch[0]
    ops.bump_weights_epoch(parameters=False)         # a training forward's running-statistics update is not a stale input
    assert train_ops._input_stamp(m) == s2 and ops._weights_epoch[0] == epoch + 1     # (prepared layouts are still rebuilt)
