"""``images.ImageCache`` / ``images.source_key`` on CPU tensors: the one staleness rule every image made from parameters is held to."""

from __future__ import annotations

import ctypes
import gc
import weakref

import pytest
import torch

from range_view_3d_detection_amd.images import ImageCache, source_key

SLOT = ("weight", "gather", "bf16")


class Maker:
    """A counting ``make``: the image is 2 x the source, written into the old entry's buffer when there is one."""

    def __init__(self, src, in_place=False):
        self.src, self.in_place, self.calls, self.olds = src, in_place, 0, []

    def __call__(self, old):
        self.calls += 1
        self.olds.append(old)
        if self.in_place and old is not None:
            return old.data.copy_(2.0 * self.src.detach())
        return 2.0 * self.src.detach()


def test_hit_serves_the_same_object_without_make():
    t = torch.arange(4.0)
    cache, make = ImageCache(), Maker(t)
    first = cache.get(SLOT, (t,), make)
    again = cache.get(SLOT, (t,), make)
    assert again is first and again.data is first.data and make.calls == 1
    assert first.slot == SLOT and first.sources == (t,) and first.key == source_key(t) and first.aux is None and not first.persistent
    assert cache.current(SLOT) is first and first.current and cache.entries() == [first]


@pytest.mark.parametrize("change", ["add_", "increment_version", "data_swap"])
def test_changes_torch_can_see_re_make(change):
    p = torch.nn.Parameter(torch.arange(4.0))
    cache, make = ImageCache(), Maker(p)
    first = cache.get(SLOT, (p,), make)
    key = source_key(p)
    with torch.no_grad():
        if change == "add_":
            p.add_(1)
        elif change == "increment_version":
            torch.autograd.graph.increment_version(p)
        else:
            version = p._version
            p.data = torch.full((4,), 7.0)
            assert p._version == version  # (the key moves on the pointer alone)
    assert source_key(p) != key and not first.current and cache.current(SLOT) is None and cache.entries() == [first]
    second = cache.get(SLOT, (p,), make)
    assert make.calls == 2 and second is not first and torch.equal(second.data, 2.0 * p.detach())
    assert cache.current(SLOT) is second and cache.get(SLOT, (p,), make) is second and make.calls == 2


def test_raw_pointer_write_does_not_re_make():
    """The documented premise of ``TapLayer.invalidate``: neither version nor pointer moves, the old image is served until ``clear()``."""
    t = torch.zeros(4)
    cache, make = ImageCache(), Maker(t)
    first = cache.get(SLOT, (t,), make)
    src = (ctypes.c_float * 4)(1.0, 2.0, 3.0, 4.0)
    ctypes.memmove(t.data_ptr(), src, ctypes.sizeof(src))
    assert t[3] == 4.0
    assert cache.get(SLOT, (t,), make) is first and make.calls == 1 and torch.equal(first.data, torch.zeros(4))
    cache.clear()
    assert cache.entries() == [] and cache.current(SLOT) is None
    assert torch.equal(cache.get(SLOT, (t,), make).data, 2.0 * t) and make.calls == 2


def test_extra_is_part_of_the_key():
    t = torch.ones(4)
    cache, make = ImageCache(), Maker(t)
    first = cache.get(SLOT, (t,), make, extra=(1e-5,))
    assert cache.get(SLOT, (t,), make, extra=(1e-5,)) is first and make.calls == 1 and first.extra == (1e-5,)
    second = cache.get(SLOT, (t,), make, extra=(1e-3,))
    assert second is not first and make.calls == 2 and second.key != first.key and second.current


def test_make_receives_the_old_entry_and_the_old_entry_is_let_go():
    t = torch.ones(4)
    cache, make = ImageCache(), Maker(t, in_place=True)
    first = cache.get(SLOT, (t,), make, persistent=True)
    buf, ptr = first.data, first.data.data_ptr()
    t.mul_(3.0)
    second = cache.get(SLOT, (t,), make)
    assert make.olds == [None, first] and second.data is buf and second.data.data_ptr() == ptr and torch.equal(buf, torch.full((4,), 6.0))
    assert second.persistent  # (written into the buffer of a persistent entry)
    assert cache.entries() == [second] and cache.current(SLOT) is second
    # a re-made slot does not keep the old entry (or, when make allocates, its buffer) reachable
    make.in_place, make.olds = False, []
    old_entry, old_buf = weakref.ref(second), weakref.ref(second.data)
    t.mul_(2.0)
    del first, second, buf
    third = cache.get(SLOT, (t,), make)
    make.olds = []
    gc.collect()
    assert old_entry() is None and old_buf() is None and cache.entries() == [third] and not third.persistent


def test_a_fresh_image_releases_the_stale_ones_of_its_kind():
    w, b = torch.ones(4), torch.ones(2)
    cache = ImageCache()
    f16 = cache.get(("weight", "gather", "f16"), (w,), Maker(w))
    kept = cache.adopt(("weight", "scatter", "bf16"), (w,), torch.zeros(4), persistent=True)
    bias = cache.get(("bias", None, "f32"), (b,), Maker(b))
    w.add_(1.0)
    b.add_(1.0)
    fresh = cache.get(SLOT, (w,), Maker(w))
    assert f16 not in cache.entries()  # stale, same kind: gone
    assert cache.held(kept.slot) is kept and not kept.current  # stale but persistent: waits to be rewritten
    assert cache.held(bias.slot) is bias  # stale, another kind: until that kind is re-made
    assert cache.current(SLOT) is fresh and len(cache.entries()) == 3


def test_adopt_marks_entries_current_and_none_sources_are_accepted():
    w = torch.ones(4)
    cache = ImageCache()
    img, aux = torch.zeros(8), torch.zeros(2)
    e = cache.adopt(SLOT, (w, None), img, aux=aux, extra=("x",), persistent=True)
    assert cache.current(SLOT) is e and e.data is img and e.aux is aux and e.persistent and e.sources == (w, None)
    assert e.key == source_key(w, None, extra=("x",)) == ((w._version, w.data_ptr()), None, "x")
    make = Maker(w)
    assert cache.get(SLOT, (w, None), make, extra=("x",)) is e and make.calls == 0
    w.add_(1.0)
    assert cache.current(SLOT) is None and cache.held(SLOT) is e
    assert cache.adopt(SLOT, (w, None), img, extra=("x",)).persistent  # (same buffer again: still the persistent one)
    none = cache.get(("bias", None, "f32"), (None,), lambda old: torch.zeros(1))
    assert none.current and none.key == (None,)
