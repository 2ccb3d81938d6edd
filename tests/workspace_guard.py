"""What the tests of the workspace and output-buffer contract (tests/test_gpu_workspace_contract.py; the harness itself is tested
on the CPU by tests/test_workspace_guard_cpu.py) plant around the memory a kernel may write:

``WorkspaceGuard``  band | a slice of EXACTLY n bytes | band, in one uint8 tensor: the slice is what a training entry gets as its
                    workspace (include/evac.h: "evac_*_workspace_bytes(..) bytes, 16-byte aligned, contents irrelevant before and
                    after"), filled with a chosen byte; every byte outside it is compared with a snapshot taken before the call.
``Guarded``         float tensors in one buffer of canaries (moved here from tests/test_gpu_transformer_update.py): what a kernel
                    writes as OUTPUT -- gradients, statistics rows, an optimiser's header -- with 64 canaries behind every one.

Both work on any device; nothing here calls the library."""
import numpy as np

DEV = "cuda:0"
CANARY = -12345.0
GUARD = 64                                       # floats between two tensors of a guarded buffer
BAND = 4096                                      # bytes in front of and behind a planted slice
BAND_BYTE = 0xA5


class WorkspaceGuard:
    """``band | slice of exactly n bytes | band`` in one uint8 tensor on ``device``, the bands ``BAND`` bytes of ``BAND_BYTE``, the
    slice filled with ``fill``.  The slice starts ``offset`` bytes past a 4096-byte boundary: 0, or 16 for the minimum alignment
    the training entries document.  ``slice`` is a uint8 view with ``numel() == n``: trainer._call_buffers and
    population._update_population take a workspace that is large enough as it is.

    ``snapshot()`` before a call, ``assert_outside_unchanged()`` after it: every byte outside the slice equals the snapshot.  A
    snapshot and not the constant, so that ``replant(m)`` can plant a SHORTER slice at the front of a workspace an earlier, larger
    call has dirtied: everything behind the first m bytes then counts as outside, the dirt included."""

    def __init__(self, n, fill=0x00, offset=0, device=DEV):
        import torch
        n, offset = int(n), int(offset)
        assert n >= 1 and 0 <= offset < BAND and offset % 16 == 0
        raw = torch.full((2 * BAND + BAND + offset + n,), BAND_BYTE, dtype=torch.uint8, device=device)
        start = BAND + (-(raw.data_ptr() + BAND)) % BAND + offset           # >= BAND bytes in front, `offset` past a boundary
        self.raw = raw                                                      # (keeps the allocation alive)
        self.buf = raw[start - BAND:start + n + BAND]                       # band | slice | band, nothing else
        self.n, self.offset = n, offset
        self.slice.fill_(int(fill))
        self.snap = None
        assert (self.slice.data_ptr() - offset) % BAND == 0 and self.slice.numel() == n

    @property
    def slice(self):
        return self.buf[BAND:BAND + self.n]

    def replant(self, n, fill=None):
        """A shorter slice at the front of the same buffer (contents kept unless ``fill`` is given); returns it."""
        n = int(n)
        assert 1 <= n <= self.n
        self.n = n
        if fill is not None:
            self.slice.fill_(int(fill))
        self.snap = None
        return self.slice

    def snapshot(self):
        self.snap = self.buf.clone()
        return self.snap

    def outside_changes(self):
        """The offsets, relative to the slice's first byte, of the bytes outside the slice that differ from the snapshot
        (negative: in front of it; >= n: behind it)."""
        import torch
        assert self.snap is not None, "snapshot() first"
        differs = self.buf != self.snap
        differs[BAND:BAND + self.n] = False
        return (torch.nonzero(differs).reshape(-1) - BAND).tolist()

    def assert_outside_unchanged(self, what=""):
        changed = self.outside_changes()
        assert not changed, (what, f"{len(changed)} bytes outside the slice of {self.n} bytes changed; offsets from its start:",
                             changed[:16])


class Guarded:
    """Copies of ``arrays`` in one device buffer of canaries, ``GUARD`` floats in front of the first and behind every one."""

    def __init__(self, arrays, device=DEV):
        import torch
        sizes = [int(a.size) for a in arrays]
        self.buf = torch.full((GUARD + sum(n + GUARD for n in sizes),), CANARY, dtype=torch.float32, device=device)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.views, at = [], GUARD
        for a, n in zip(arrays, sizes):
            v = self.buf[at:at + n]
            v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            self.mask[at:at + n] = False
            self.views.append(v)
            at += n + GUARD

    def ptrs(self):
        return [v.data_ptr() for v in self.views]

    def canaries_intact(self):
        return bool((self.buf[self.mask] == CANARY).all())

    def host(self, shapes):
        return [v.cpu().numpy().reshape(s) for v, s in zip(self.views, shapes)]
