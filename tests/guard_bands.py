"""Guard-band arenas for the memory-extent tests (tests/test_gpu_memory_extents.py, tests/test_memory_extents_cpu.py): every buffer a C ABI
call gets - input, output, workspace - is a view into ONE backing uint8 tensor, with a band of a fixed byte pattern before and after it.
After the call `Arena.check()` finds any store outside the buffers (a tile row past a ragged end, a size query that reports too little)
and any change of a read-only input.  A plain module like gpu_helpers.py: not collected, no tests of its own, no device work at import."""
import torch

PATTERN = 0xA5          # neither 0x00 nor 0xFF: as float32 -2.87e-16, as int32 -1515870811, as int64 -6510615555426900571
ALIGN = 256             # every buffer starts on a 256-byte boundary of the address space, as torch's own allocations do
# Width of the band before and after every buffer.  A stray store lands in a band - and is seen - as long as it stays within this distance of
# the buffer it belongs to, so the band must cover the largest block one workgroup stores per iteration at the tested shapes:
#   - 1 KiB: one MFMA fragment (the packer, the sigma' planes of the reverse sweep, a plane of the sweep's slab);
#   - 384 B: a point tile of 32 points x 12 B (grad3 of the value + gradient kernels), 3 KiB for a 256-point launch tile;
#   - 8 KiB: one ray's 1024 samples x 8 B of int64 indices / permutation; 12 KiB for its gradients_flip row (1024 x 12 B);
#   - 272 KiB + 258 KiB: the A and Z blocks one tile of 32 points leaves in the training backward's stash for the d8w256L10 network
#     (build_vjp_layout: a_tile_kb, z_tile_kb - the "~0.54 MiB per tile" of emap_common.h), the largest of all.
# 1 MiB covers a whole stash tile (A + Z) and is far above the 64 KiB floor.
GUARD_BYTES = 1 << 20

_INT_SENTINEL = {torch.int32: -1515870811, torch.int64: -6510615555426900571, torch.uint8: PATTERN}


class GuardError(AssertionError):
    pass


class Arena:
    """Buffers with guard bands from one backing uint8 tensor: [guard][buffer][guard][buffer] ... [guard] - neighbours share a band.

        a = Arena("cuda:0", capacity=64 << 20)
        x = a.frozen(x_cpu)                      # read-only input: guarded, and compared bit for bit by check()
        out = a.buf((P, 3), torch.float32, fill="nan", name="grad3")
        ws = a.bytes(nbytes, fill="pattern", name="workspace")      # exactly nbytes long
        ... the call, a synchronise ...
        a.check(); a.check_written(out)
    """

    def __init__(self, device, capacity=32 << 20):
        self.device = torch.device(device)
        self.backing = torch.full((int(capacity) + ALIGN,), PATTERN, dtype=torch.uint8, device=self.device)
        self.base = (-self.backing.data_ptr()) % ALIGN      # offset of the first 256-byte boundary inside the backing tensor
        self.top = self.base                                # end of the last buffer (the next band starts here)
        self.entries = []                                   # (name, start, nbytes) in backing-tensor offsets
        self.inputs = []                                    # (name, view, pristine copy)

    # ---- handing out ---------------------------------------------------------------------------
    def _take(self, nbytes, name):
        start = self.top + GUARD_BYTES
        start += (self.base - start) % ALIGN
        end = start + nbytes
        if end + GUARD_BYTES > self.backing.numel():
            raise RuntimeError(f"Arena: capacity {self.backing.numel()} too small for {name!r} ({nbytes} bytes at {start})")
        self.entries.append((name or f"buf{len(self.entries)}", start, nbytes))
        self.top = end
        return self.backing[start:end]

    def buf(self, shape, dtype=torch.float32, fill="zero", name=None):
        """A contiguous view of `shape` / `dtype` on a 256-byte boundary.  fill: "zero", "pattern" (every byte 0xA5), "nan" (float: NaN;
        integer: the pattern's value - the sentinel check_written looks for), or a tensor whose values are copied in."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = 1
        for s in shape:
            n *= int(s)
        es = torch.empty((), dtype=dtype).element_size()
        raw = self._take(n * es, name)
        v = raw.view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=self.device)
        if isinstance(fill, torch.Tensor):
            v.copy_(fill.to(dtype).reshape(shape))
        elif fill == "zero":
            raw.zero_()
        elif fill == "nan" and dtype.is_floating_point:
            v.fill_(float("nan"))
        elif fill not in ("pattern", "nan"):
            raise ValueError(fill)
        return v

    def bytes(self, n, fill="zero", name=None):
        """A uint8 view of exactly n bytes (a workspace of the queried size: the same n goes to the call as workspace_bytes)."""
        return self.buf((int(n),), torch.uint8, fill, name or "workspace")

    def frozen(self, tensor, name=None):
        """`tensor` as a read-only input inside the arena: check() also asserts that it still holds the same bits."""
        t = tensor.detach()
        v = self.buf(t.shape, t.dtype, fill=t, name=name or f"input{len(self.inputs)}")
        self.inputs.append((self.entries[-1][0], v, v.clone()))
        return v

    # ---- checking ------------------------------------------------------------------------------
    def _bands(self):
        """(buffer name, side, first byte, one past the last byte) of every band, in backing-tensor offsets"""
        out = []
        for i, (name, start, nbytes) in enumerate(self.entries):
            lo = self.entries[i - 1][1] + self.entries[i - 1][2] if i else max(start - GUARD_BYTES, 0)
            out.append((name, "before", max(lo, start - GUARD_BYTES), start))
            out.append((name, "after", start + nbytes, start + nbytes + GUARD_BYTES))
        return out

    def violations(self):
        """A list of messages: every touched band (buffer, side, offsets of the first and last changed byte relative to the buffer's edge:
        'before' counts back from the buffer's first byte, -1 is the byte just before it; 'after' counts from its end, +0 is the byte just
        after it) and every changed frozen input."""
        bands = self._bands()
        msgs = []
        if bands:
            counts = torch.stack([(self.backing[a:b] != PATTERN).sum() for _, _, a, b in bands]).tolist()
            for (name, side, a, b), c in zip(bands, counts):
                if not c:
                    continue
                idx = torch.nonzero(self.backing[a:b] != PATTERN).reshape(-1)
                first, last = int(idx[0]), int(idx[-1])
                if side == "before":
                    first, last = first - (b - a), last - (b - a)
                msgs.append(f"guard {side} buffer '{name}' touched: {c} byte(s), first at {first:+d}, last at {last:+d} relative to the "
                            f"buffer's {'start' if side == 'before' else 'end'}")
        for name, v, keep in self.inputs:
            a, b = v.reshape(-1).view(torch.uint8), keep.reshape(-1).view(torch.uint8)
            if not torch.equal(a, b):
                idx = torch.nonzero(a != b).reshape(-1)
                msgs.append(f"read-only input '{name}' changed: {idx.numel()} byte(s), first at byte {int(idx[0])}, last at byte {int(idx[-1])}")
        return msgs

    def check(self):
        msgs = self.violations()
        if msgs:
            raise GuardError("; ".join(msgs))

    @staticmethod
    def check_written(view, name="output"):
        """No sentinel of a "nan" prefill is left: the call wrote every element."""
        if view.dtype.is_floating_point:
            left = torch.isnan(view)
        else:
            left = view == _INT_SENTINEL[view.dtype]
        n = int(left.sum())
        if n:
            idx = torch.nonzero(left.reshape(-1)).reshape(-1)
            raise GuardError(f"'{name}': {n} of {view.numel()} element(s) still hold the prefill sentinel, first at flat index {int(idx[0])}, "
                             f"last at {int(idx[-1])}")
