"""One keyed cache for every image made from parameters (packed weights of both operand types, folded forms, eval-mode BatchNorm folds,
padded biases): one record, ``Image``, and one staleness rule, ``source_key``.  Plain torch, no library calls: CPU tensors work too.
The rule sees what torch sees -- in-place ops, ``copy_``, ``load_state_dict``, ``torch.autograd.graph.increment_version``, a tensor swapped
in through ``.data``.  A write through the raw pointer moves neither version nor pointer: ``ImageCache.clear`` is for that."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

from torch import Tensor


def source_key(*tensors: Optional[Tensor], extra: Sequence = ()) -> tuple:
    """(version, pointer) of every source tensor (None: a layer without a bias), then ``extra``: plain values the image depends on."""
    return tuple(None if t is None else (t._version, t.data_ptr()) for t in tensors) + tuple(extra)


@dataclass
class Image:  # slot = (kind, form, operand tag), kind in weight / folded / eval_fold / bias
    slot: tuple
    key: tuple  # source_key(*sources, extra=extra) when ``data`` was written
    sources: tuple  # the tensors it was made from: an auditor re-makes the image from these
    data: Tensor
    aux: Optional[Tensor] = None  # the eval fold's bias
    persistent: bool = False  # the buffer outlives staleness and is rewritten in place (batched re-pack, bf16 folded image)
    extra: tuple = ()

    @property
    def current(self) -> bool:
        return self.key == source_key(*self.sources, extra=self.extra)


class ImageCache:
    def __init__(self) -> None:
        self._entries: Dict[tuple, Image] = {}

    def held(self, slot: tuple) -> Optional[Image]:
        return self._entries.get(slot)

    def current(self, slot: tuple) -> Optional[Image]:
        e = self._entries.get(slot)
        return e if e is not None and e.current else None

    def entries(self) -> List[Image]:
        return list(self._entries.values())

    def clear(self) -> None:
        self._entries.clear()

    def adopt(self, slot: tuple, sources: Sequence, data: Tensor, aux: Optional[Tensor] = None, extra: Sequence = (), persistent: bool = False) -> Image:
        """Store ``data``, just written from ``sources``, as the current image of ``slot``.  An image written into the buffer of a
        persistent entry stays persistent.  The stale images of the same kind go (a changed parameter keeps no fp16 or eval images
        beside the new ones); persistent ones wait to be rewritten."""
        old = self._entries.get(slot)
        persistent = persistent or (old is not None and old.persistent and old.data is data)
        for s, e in list(self._entries.items()):
            if s[0] == slot[0] and not e.persistent and not e.current:
                del self._entries[s]
        e = self._entries[slot] = Image(slot, source_key(*sources, extra=extra), tuple(sources), data, aux, persistent, tuple(extra))
        return e

    def get(self, slot: tuple, sources: Sequence, make: Callable[[Optional[Image]], object], extra: Sequence = (), persistent: bool = False) -> Image:
        """The image of ``slot`` if it was made from ``sources`` as they are now; otherwise what ``make(old entry or None)`` returns --
        the image, or (image, aux); it may write into the old entry's buffer -- takes its place."""
        e = self._entries.get(slot)
        if e is None or e.key != source_key(*sources, extra=extra):
            made = make(e)
            e = self.adopt(slot, sources, *(made if isinstance(made, tuple) else (made, None)), extra, persistent)
        return e
