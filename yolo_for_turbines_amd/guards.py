"""Who declares host-side state that recorded an address stale: one check, shared by the eval fast path
(`ModelState.refresh_weights`) and the training launch tables (`TrainPlan`)."""
from __future__ import annotations


class SlotGuard:
    """Remembers what sits in a list of (owner dict, key) slots and tells whether all of it is still there.

    tensors: slots of a module's `_parameters` / `_buffers` (an entry that is None is remembered as a plain value).
    `ok()` re-reads every slot's CURRENT entry: it must be the remembered tensor object at the remembered address, so a
    replaced Parameter or buffer object fails `is` even though the old tensor, kept alive here, never moved.
    versions=True: the tensor's `_version` must not have moved either (eval: nothing wrote it; training writes every
    tensor each step and leaves this off). values: slots of plain values (a module's `__dict__`) that must compare equal."""

    def __init__(self, tensors, versions=False, values=()):
        self.versions = versions
        self.tensors = []                 # flat (owner, key, tensor, version, address): no Python object per check beyond these
        self.values = []                  # (owner, key, value)
        for owner, key in tensors:
            t = owner[key]
            if t is None:
                self.values.append((owner, key, None))
            else:
                self.tensors.append((owner, key, t, t._version, t.data_ptr()))
        self.values += [(owner, key, owner[key]) for owner, key in values]

    def ok(self):
        if self.versions:
            for owner, key, t, ver, ptr in self.tensors:
                if owner[key] is not t or t._version != ver or t.data_ptr() != ptr:
                    return False
        else:
            for owner, key, t, ver, ptr in self.tensors:
                if owner[key] is not t or t.data_ptr() != ptr:
                    return False
        for owner, key, v in self.values:
            cur = owner[key]
            if cur is not v and cur != v:
                return False
        return True
