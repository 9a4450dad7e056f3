"""One per-step list of a model (f_star[i], Sigma[i], ... one entry per LDS step in the reference): the list
knows when it changed."""
from collections.abc import MutableSequence
from itertools import count

import torch

_stamps = count(1)          # one counter per process: two lists never share a stamp, and a stamp never comes back


class StepList(MutableSequence):
    """A per-step list held either as ONE stacked device tensor [L, ...] or as a real Python list of tensors.  Reads behave like
    the reference's list (len, [i], [-1], slices, iteration, ``+``); the first mutation of a stacked one turns it into a real list
    (copy-on-write), so a model and its copies can share one stack.  A 2 272-step chain is 8 such lists: building 18 000 tensor
    objects per pass, and re-stacking them for every batched kernel, was 10 % of the offline loop's wall-clock.

    ``stamp`` is an integer drawn from the process-wide counter at construction and again at EVERY mutation (item and slice
    assignment, del, insert, append and what MutableSequence builds on them: pop, extend, +=, reverse, clear, remove); reads never
    change it.  Whatever is derived from the list - its own ``stack()`` first of all - is valid exactly as long as the stamp it was
    computed at is still the list's stamp.  Writing INTO a tensor the list holds is invisible to it: say ``touch()``.

    torch.stack / torch.cat only take real lists and tuples: pass ``list(m.f_star)`` or use ``m.f_star.stack()``."""
    __slots__ = ("_st", "_ls", "stamp", "_stacked", "_sym")

    def __init__(self, items=()):
        """items: a stacked tensor [L, ...] (kept, not copied), or a list, which is taken as it is (any other iterable is
        copied into one)."""
        if torch.is_tensor(items):
            self._st, self._ls = items, None
        else:
            self._st, self._ls = None, items if type(items) is list else list(items)
        self.touch()

    def touch(self):
        """The list changed: a new stamp, and what was cached with the old one is dropped."""
        self.stamp, self._stacked, self._sym = next(_stamps), None, None

    def _list(self):
        """The real list, for a mutation."""
        if self._ls is None:
            self._ls, self._st = list(self._st.unbind(0)), None
        self.touch()
        return self._ls

    def stacked(self):
        """The tensor [L, ...] the list was built over while it still is that tensor's view (no mutation since), else None."""
        return self._st

    def stack(self):
        """The entries as one contiguous tensor [L, ...]: the underlying tensor itself while stacked, else stacked once per
        stamp.  Read-only for the caller."""
        if self._ls is None:
            return self._st
        if self._stacked is None or self._stacked[0] != self.stamp:
            self._stacked = (self.stamp, torch.stack(self._ls).contiguous())
        return self._stacked[1]

    def symmetric(self):
        """Is every matrix of the stack equal to its transpose bit for bit?  One device check per stamp."""
        if self._sym is None or self._sym[0] != self.stamp:
            S = self.stack()
            self._sym = (self.stamp, bool(torch.equal(S, S.transpose(1, 2))))
        return self._sym[1]

    def __len__(self):
        return self._st.shape[0] if self._ls is None else len(self._ls)

    def __getitem__(self, i):
        if self._ls is not None:
            return self._ls[i]
        if isinstance(i, slice):
            return list(self._st[i].unbind(0))
        return self._st[i]

    def __setitem__(self, i, v):
        self._list()[i] = v

    def __delitem__(self, i):
        del self._list()[i]

    def insert(self, i, v):
        self._list().insert(i, v)

    def append(self, v):
        self._list().append(v)

    def __iter__(self):
        return iter(self._st.unbind(0) if self._ls is None else self._ls)

    def __add__(self, other):
        return list(self) + list(other)

    def __radd__(self, other):
        return list(other) + list(self)

    def copy(self):
        """A list of its own over the same entries (a stacked one shares the stack until either side is mutated)."""
        if self._ls is None:
            return StepList(self._st)
        new = StepList(list(self._ls))
        if self._stacked is not None and self._stacked[0] == self.stamp:        # same entries: the same stack serves the copy
            new._stacked = (new.stamp, self._stacked[1])
        return new
