"""Who holds a module's training workspace between a node's forward and its backward.

A ``_TrainStep`` node (``train_ops``) leaves its activations, BatchNorm scale / shift and pooled context in a workspace and
reads them back in its backward.  ``LeasePool`` hands every forward a workspace nobody else holds: the module's own one
(``primary``) when it is free -- the ordinary loop never sees another -- else a spare.  The node gives it back at the end of
its backward; a node that never runs one gives it back when its ``ctx`` (the lease's only owner) is collected.

Only bookkeeping lives here: a slot is any object (``ops.Workspace`` in ``train_ops``, a stand-in in the host tests), and no
torch or device call is made.
"""
import itertools
import weakref

_tickets = itertools.count(1)


class Lease:
    """One node's hold on one slot.  ``shared``: another node of the module was live at some point of this node's life, so
    its parameter gradients must leave the backward as tensors of their own (``train_ops``: clones of the flat buffer)."""
    __slots__ = ("pool", "slot", "ticket", "shared", "released", "__weakref__")

    def __init__(self, pool, slot, shared):
        self.pool, self.slot, self.shared, self.released = pool, slot, shared, False
        self.ticket = slot.lease_ticket = next(_tickets)

    def moved_on(self):
        """True once the slot was handed to another forward after this lease gave it back: what this node left there is gone."""
        return self.released and self.slot.lease_ticket != self.ticket

    def check(self):
        if self.moved_on():
            raise RuntimeError("retain_graph: backward again after another forward on this model -- the workspace that held "
                               "this node's activations was given back at the end of its first backward and has since been "
                               "reused; run the forward again (a second backward with no forward in between works)")

    def release(self):
        if not self.released:
            self.released = True
            self.pool._give_back(self)

    def __del__(self):
        try:
            self.release()
        except Exception:                # (interpreter shutdown: the pool may be half gone)
            pass


class LeasePool:
    """The slots of one module.  ``primary`` is taken whenever it is free; spares are made by ``new_slot()`` while it is
    held, wait in ``free`` while any node is live and are dropped (their memory with them) when the last one has finished."""

    def __init__(self, primary, new_slot):
        self.primary, self.new_slot = primary, new_slot
        self.primary_held = False
        self.free = []
        self.live = weakref.WeakSet()

    def take(self):
        shared = False
        for other in self.live:
            other.shared = shared = True
        if not self.primary_held:
            slot, self.primary_held = self.primary, True
        else:
            slot = self.free.pop() if self.free else self.new_slot()
        lease = Lease(self, slot, shared)
        self.live.add(lease)
        return lease

    def _give_back(self, lease):
        self.live.discard(lease)
        if lease.slot is self.primary:
            self.primary_held = False
        else:
            self.free.append(lease.slot)
        if not self.live:
            self.free.clear()
