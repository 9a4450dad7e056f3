"""hdpgpc_amd/steplist.py on CPU tensors: the stamp moves at every mutation and at no read, stack() follows the entries (a
rewritten MIDDLE entry included), a stacked list hands out its own tensor, copies are independent."""
import pytest
import torch

from hdpgpc_amd.steplist import StepList

L, T = 5, 3


def _entries(seed=0):
    return torch.arange(L * T * T, dtype=torch.float64).reshape(L, T, T) + 100.0 * seed


def _new(v=7.0):
    return torch.full((T, T), v, dtype=torch.float64)


def _both():
    """The same five entries in stack mode and in list mode."""
    return [("stack", StepList(_entries())), ("list", StepList(list(_entries().unbind(0))))]


MUTATORS = {
    "set_first": lambda a: a.__setitem__(0, _new()),
    "set_middle": lambda a: a.__setitem__(2, _new()),
    "set_last": lambda a: a.__setitem__(-1, _new()),
    "slice_first": lambda a: a.__setitem__(slice(0, 1), [_new()]),
    "slice_middle": lambda a: a.__setitem__(slice(1, 3), [_new(), _new(8.0)]),
    "slice_last": lambda a: a.__setitem__(slice(L - 1, L), [_new()]),
    "del": lambda a: a.__delitem__(1),
    "insert": lambda a: a.insert(2, _new()),
    "append": lambda a: a.append(_new()),
    "extend": lambda a: a.extend([_new(), _new(8.0)]),
    "pop": lambda a: a.pop(),
    "iadd": lambda a: a.__iadd__([_new()]),
    "reverse": lambda a: a.reverse(),
    "clear": lambda a: a.clear(),
}
READS = {
    "len": len,
    "index": lambda a: (a[0], a[2], a[-1]),
    "slice": lambda a: a[1:3],
    "iter": lambda a: [t for t in a],
    "add": lambda a: (a + [_new()], [_new()] + a),
    "copy": lambda a: a.copy(),
    "stack": lambda a: a.stack(),
    "symmetric": lambda a: a.symmetric(),
}


@pytest.mark.parametrize("name", sorted(MUTATORS))
def test_every_mutator_changes_the_stamp(name):
    for mode, a in _both():
        want = list(a)
        MUTATORS[name](want)                       # the same operation on a plain list
        seen = {a.stamp}
        a.stack()
        before = a.stamp
        MUTATORS[name](a)
        assert a.stamp != before and a.stamp not in seen, (name, mode)
        assert len(a) == len(want) and all(torch.equal(x, y) for x, y in zip(a, want)), (name, mode)
        if len(want):
            assert torch.equal(a.stack(), torch.stack(want)), (name, mode)     # and the cached stack went with the stamp


@pytest.mark.parametrize("name", sorted(READS))
def test_no_read_changes_the_stamp(name):
    for mode, a in _both():
        before = a.stamp
        READS[name](a)
        READS[name](a)
        assert a.stamp == before, (name, mode)
        assert torch.equal(a.stack(), _entries()), (name, mode)


def test_stack_after_a_middle_entry_assignment_holds_the_new_values():
    """(length, identity of the last entry) - the key the stacks were cached under before - does not see this one."""
    for mode, a in _both():
        first = a.stack()
        last = a[-1] if mode == "list" else None
        a[2] = _new(-1.0)
        want = _entries()
        want[2] = -1.0
        assert len(a) == L and (last is None or a[-1] is last)
        assert torch.equal(a.stack(), want), mode
        assert torch.equal(first, _entries()), mode              # the stack handed out earlier was not written into


def test_stack_twice_is_the_same_tensor_object():
    for mode, a in _both():
        assert a.stack() is a.stack(), mode
        a[1] = _new()
        s = a.stack()
        assert a.stack() is s and a.symmetric() == a.symmetric(), mode


def test_stack_mode_hands_out_the_constructors_tensor():
    st = _entries()
    a = StepList(st)
    assert a.stack() is st and a.stack().data_ptr() == st.data_ptr()
    assert a[1].data_ptr() == st[1].data_ptr() and a.copy().stack().data_ptr() == st.data_ptr()


def test_a_list_is_taken_as_it_is():
    lst = list(_entries().unbind(0))
    a = StepList(lst)
    assert a[0] is lst[0] and a[-1] is lst[-1] and a[1:3][0] is lst[1]
    assert len(StepList()) == 0 and len(StepList(tuple(lst))) == L


def test_symmetric():
    sym = _entries() + _entries().transpose(1, 2)
    for a in (StepList(sym), StepList(list(sym.unbind(0)))):
        assert a.symmetric() is True
        a[2] = _entries()[1]                                       # a middle entry that is not symmetric
        assert a.symmetric() is False
        a[2] = sym[0]
        assert a.symmetric() is True


def test_touch_publishes_a_write_into_a_held_tensor():
    a = StepList(list(_entries().unbind(0)))
    old, before = a.stack(), a.stamp
    a[2].fill_(-3.0)
    assert a.stack() is old                                        # invisible to the list ...
    a.touch()
    assert a.stamp != before and bool((a.stack()[2] == -3.0).all())     # ... until it is told


def test_copy_on_write():
    for mode, a in _both():
        a.stack()
        stamp = a.stamp
        b = a.copy()
        assert isinstance(b, StepList) and b.stamp != stamp
        assert torch.equal(b.stack(), a.stack())
        b[1] = _new()
        b.append(_new(9.0))
        del b[0]
        assert a.stamp == stamp and len(a) == L, mode
        assert torch.equal(a.stack(), _entries()) and all(torch.equal(x, y) for x, y in zip(a, _entries())), mode
        assert len(b) == L and torch.equal(b[0], _new()) and torch.equal(b[-1], _new(9.0)), mode
        assert torch.equal(b.stack(), torch.stack(list(b))), mode


def test_stamps_are_distinct_and_never_repeat():
    lists = [StepList(_entries()) for _ in range(4)] + [StepList(list(_entries().unbind(0))) for _ in range(4)] + [StepList()]
    lists += [x.copy() for x in lists]
    seen = [x.stamp for x in lists]
    assert len(set(seen)) == len(seen) and all(type(s) is int for s in seen)
    for x in lists:
        for _ in range(3):
            x.append(_new())
            assert x.stamp not in seen
            seen.append(x.stamp)
            x[0] = _new()
            assert x.stamp not in seen
            seen.append(x.stamp)
    del lists[0]                                                    # a freed list's stamp (unlike its address) is not handed out again
    assert StepList(_entries()).stamp not in seen
