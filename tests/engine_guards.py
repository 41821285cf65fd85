"""The engine's real call sites under guards: while ``guarded()`` is active, GeneratorEngine._empty hands out every work buffer
inside an allocation with guard rows (2-D matrices: GUARD_ROWS poisoned rows on both sides, same row stride) or guard elements
(other shapes) around it, and engine._Arena puts guard doubles around the statistics arena.  ``violations()`` lists the buffers
whose guards are no longer bit-intact.  Nothing in engine.py changes; only the guards are kept and compared, not the buffers."""
import torch

from kernel_cases import GUARD_ROWS, _poison
from uda_clr_amd import engine

GUARD_ELEMS = 4096          # flat guards, in elements: a multiple of 4, so a 16-byte aligned tensor stays 16-byte aligned
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    return t.reshape(-1).view(_INT[t.element_size()])


class guarded:
    def __enter__(self):
        self.held = []              # (name, allocation, [(guard view, snapshot of its bits)])
        self.keep_empty, self.keep_arena = engine.GeneratorEngine.__dict__["_empty"], engine._Arena
        outer = self

        def _empty(x, *shape, dtype=torch.float32):
            if len(shape) == 2:
                P, ld = shape
                base = torch.empty(P + 2 * GUARD_ROWS, ld, dtype=dtype, device=x.device)
                if dtype == torch.float32:       # guards always hold the by-row poison; the matrix itself as the engine would fill it
                    _poison(base[:GUARD_ROWS])
                    _poison(base[GUARD_ROWS + P:])
                    if engine.POISON_BUFFERS:
                        _poison(base[GUARD_ROWS:GUARD_ROWS + P])
                else:
                    base.view(torch.uint8)[:] = 0xA5
                t = base[GUARD_ROWS:GUARD_ROWS + P]
                guards = [base[:GUARD_ROWS], base[GUARD_ROWS + P:]]
            else:
                n = 1
                for d in shape:
                    n *= d
                base = torch.empty(n + 2 * GUARD_ELEMS, dtype=dtype, device=x.device)
                base.view(torch.uint8)[:] = 0xA5
                t = base[GUARD_ELEMS:GUARD_ELEMS + n].view(shape)
                guards = [base[:GUARD_ELEMS], base[GUARD_ELEMS + n:]]
            assert t.data_ptr() % 16 == 0 or (len(shape) == 2 and shape[1] % 4)
            outer._hold("buffer %d %s" % (len(outer.held), list(shape)), base, guards)
            return t

        class _Arena(self.keep_arena):
            def __init__(self, like, n_doubles):
                big = torch.zeros(n_doubles + 2 * GUARD_ELEMS, dtype=torch.float64, device=like.device)
                guards = [big[:GUARD_ELEMS], big[GUARD_ELEMS + n_doubles:]]
                for gd in guards:
                    gd.view(torch.uint8)[:] = 0xA5
                self.buf, self.off = big[GUARD_ELEMS:GUARD_ELEMS + n_doubles], 0
                outer._hold("statistics arena %d (%d doubles)" % (len(outer.held), n_doubles), big, guards)

        engine.GeneratorEngine._empty = staticmethod(_empty)
        engine._Arena = _Arena
        return self

    def _hold(self, name, base, guards):
        self.held.append((name, base, [(gd, _bits(gd).clone()) for gd in guards]))

    def __exit__(self, *exc):
        engine.GeneratorEngine._empty = self.keep_empty
        engine._Arena = self.keep_arena
        return False

    def counts(self):
        """(work buffers, arenas) handed out"""
        arenas = sum(name.startswith("statistics arena") for name, _, _ in self.held)
        return len(self.held) - arenas, arenas

    def violations(self):
        """[(buffer name, "before" | "behind", first changed element of that guard)]"""
        out = []
        for name, _, guards in self.held:
            for side, (gd, snap) in zip(("before", "behind"), guards):
                d = _bits(gd) != snap
                if bool(d.any()):
                    out.append((name, side, int(d.nonzero()[0])))
        return out
