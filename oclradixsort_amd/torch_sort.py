"""torch front end of the typed sorts: what `torch.sort` / `torch.argsort` return for a 1-D tensor, computed by the HIP
back-end on torch's own stream.

    s = TorchSorter()                       # one adlhip_device on the stream that is torch's current one NOW + its scratch
    values, indices = s.sort(t)             # t: 1-D CUDA tensor, int32 / int64 / float32 / float64
    indices = s.argsort(t, descending=True)
    values, indices = s.topk(t, 10)         # the 10 largest, largest first; ties to the lower index
    values, indices = s.topk_rows(m, 10)    # m: 2-D or more; the same along the last dimension of every row
    values, indices = s.sort_rows(m)        # torch.sort(m, dim=-1, stable=True) for m of 2 dimensions or more; argsort_rows: the indices
    u, inverse, counts = s.unique(t, return_inverse=True, return_counts=True)   # torch.unique(t) on any number of dimensions
    u, counts = s.unique_consecutive(t, return_counts=True)                      # torch.unique_consecutive(t), 1-D
    u, sums = s.reduce_by_key(keys, values, op="sum")                            # per distinct key: sum / min / max of its values
    u, sums = s.reduce_consecutive(keys, values, op="sum")                       # the same per run of adjacent equal keys
    c = s.cumsum(t); m = s.cummax(t); m = s.cummin(t)                            # prefix sum / max / min, in t's dtype
    r = s.scan_by_key(keys, values, op="sum", exclusive=False, init=None)        # the same within every run of adjacent equal keys
    sel = s.masked_select(t, mask); pos = s.nonzero(mask)                        # torch.masked_select / torch.nonzero (bool or uint8 mask)
    sel = s.select_if(t, "lt", x)                                                # t[t < x], in totalOrder; also "le", "gt", "ge", "eq", "ne"
    out, count = s.partition(t, mask)                                            # the selected elements, then the others; both in input order
    c = s.bincount(t); c = s.histogram(t, edges); c = s.histc(t, 100, 0.0, 1.0)  # torch.bincount / numpy.histogram(t, edges)[0] / the same on linspace edges
    m = s.merge(a, b); m, v, i = s.merge(a, b, values=(va, vb), return_indices=True)   # torch.sort(torch.cat((a, b)), stable=True) of sorted a, b
    i = s.intersect(a, b); u = s.union(a, b); d = s.difference(a, b); x = s.symmetric_difference(a, b)   # of sorted a, b: numpy.intersect1d / union1d / setdiff1d / setxor1d
    pos = s.searchsorted(sorted_t, values, right=False); b = s.bucketize(values, boundaries)   # torch.searchsorted / torch.bucketize on a 1-D sorted tensor
    ia, ib = s.join(a, b, how="inner"); r = s.repeat_interleave(values, repeats)    # all pairs of equal elements of sorted a, b; torch.repeat_interleave
    s.close()

Always out of place and always stable.  The ONE difference from `torch.sort(t, stable=True)`: floats are ordered by
IEEE-754 totalOrder, so NaNs with the sign bit set sort FIRST (torch puts every NaN last) and -0 sorts before +0 (torch
treats them as equal and keeps their input order).  Inputs without NaN and -0 give torch's result bit for bit.

A sorter is bound to the stream that was torch's current stream on its device when it was constructed (as dist._Stage is): its sorts
are enqueued there.  Calling it while another stream is current (`with torch.cuda.stream(other)`) would leave the sort unordered
against the producer of its input and against the caching allocator, so sort() / argsort() raise RuntimeError then; make one sorter
per stream.

torch and the HIP back-end must share one HIP runtime (they share a stream).  A torch wheel that bundles its own runtime has to be
imported before the back-end's library is loaded -- `import torch` before the first oclradixsort_amd call, as dist.py does --;
TorchSorter refuses to start when torch cannot see the device.
"""
import numpy as np
import torch

from ._lib import AdlHipError
from .adl import Buffer, Config, DeviceUtils
from .pprims import Pprims

_NP_DTYPE = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}


class TorchSorter:
    def __init__(self, device_index=0):
        if not torch.cuda.is_available():
            raise AdlHipError("TorchSorter: torch sees no GPU (if the HIP back-end was used before torch was imported, the process "
                              "holds two HIP runtimes: import torch first)")
        self.torch_device = torch.device("cuda", int(device_index))
        with torch.cuda.device(self.torch_device):
            raw = torch.cuda.current_stream().cuda_stream
        self.raw_stream = raw
        self.device = DeviceUtils.allocate(cfg=Config(int(device_index)), stream=raw)
        self.pprims = Pprims()

    def close(self):
        if self.device is not None:
            torch.cuda.synchronize(self.torch_device)   # the scratch may still be in use by enqueued sorts
            self.pprims.close()
            DeviceUtils.deallocate(self.device)
            self.device = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, t):
        if not isinstance(t, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(t).__name__)
        if t.dtype not in _NP_DTYPE:
            raise TypeError("TorchSorter: dtype %s unsupported (int32, int64, float32, float64)" % t.dtype)
        if t.dim() != 1:
            raise ValueError("TorchSorter: 1-D tensors only, got %d dimensions" % t.dim())
        if t.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (t.device, self.torch_device))
        if t.numel() >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")

    @staticmethod
    def _aligned(t):
        """t contiguous and on a 16-byte boundary, as the ABI wants its inputs: a copy only for a strided input or for a view that
        starts at an odd offset (t[1:]); the input is never written"""
        src = t.contiguous()
        if src.data_ptr() % 16:
            src = src.clone()
        return src

    def _wrap(self, t, dtype):
        b = Buffer(dtype=dtype)
        b.setRawPtr(self.device, t.data_ptr(), t.numel())
        return b

    def _run(self, t, descending, want_values):
        self._check(t)
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        n = t.numel()
        src = self._aligned(t)
        values = torch.empty(n, dtype=t.dtype, device=t.device) if want_values else None
        if n == 0:
            return values, torch.empty(0, dtype=torch.int64, device=t.device)
        npdt = _NP_DTYPE[t.dtype]
        idx32 = torch.empty(n, dtype=torch.int32, device=t.device)   # uint32 positions in an int32 tensor
        lib_idx = self._wrap(idx32, np.uint32)
        p = self.pprims
        p.argsort(self.device, self._wrap(src, npdt), n, descending=descending,
                  keysOut=self._wrap(values, npdt) if want_values else None, indexOut=lib_idx)
        # the stream is synchronised by torch, never by adlhip_sync: pick up device-side faults of earlier, completed sorts
        self.device.checkFault()
        return values, idx32.to(torch.int64) & 0xffffffff

    def topk(self, t, k, largest=True, sorted=True):
        """(values, indices) like torch.topk(t, k, largest=largest, sorted=True); indices are int64.  sorted=False is accepted and
        still returns sorted output.  Ties go to the lower index: indices equal
        torch.sort(t, descending=largest, stable=True).indices[:k] (torch.topk leaves the tie order unspecified)."""
        self._check(t)
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        n, k = t.numel(), int(k)
        if k < 0 or k > n:
            raise ValueError("TorchSorter.topk: k = %d outside [0, numel = %d]" % (k, n))
        values = torch.empty(k, dtype=t.dtype, device=t.device)
        if k == 0:
            return values, torch.empty(0, dtype=torch.int64, device=t.device)
        src = self._aligned(t)
        npdt = _NP_DTYPE[t.dtype]
        idx32 = torch.empty(k, dtype=torch.int32, device=t.device)   # uint32 positions in an int32 tensor
        self.pprims.topk(self.device, self._wrap(src, npdt), n, k, descending=bool(largest), keysOut=self._wrap(values, npdt),
                         indexOut=self._wrap(idx32, np.uint32))
        self.device.checkFault()
        return values, idx32.to(torch.int64) & 0xffffffff

    def topk_rows(self, t, k, largest=True, sorted=True):
        """(values, indices) like torch.topk(t, k, dim=-1, largest=largest, sorted=True) for t.dim() >= 2: top-k along the last
        dimension, the leading dimensions flattened to rows; both results have shape t.shape[:-1] + (k,), indices are int64.
        sorted=False is accepted and still returns sorted output.  Ties go to the lower index: indices equal
        torch.sort(t, dim=-1, descending=largest, stable=True).indices[..., :k].  A 1-D tensor is topk()'s."""
        if not isinstance(t, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(t).__name__)
        if t.dtype not in _NP_DTYPE:
            raise TypeError("TorchSorter: dtype %s unsupported (int32, int64, float32, float64)" % t.dtype)
        if t.dim() < 2:
            raise ValueError("TorchSorter.topk_rows: 2-D tensors and above, got %d dimensions (topk serves 1-D)" % t.dim())
        if t.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (t.device, self.torch_device))
        cols, k = t.shape[-1], int(k)
        if cols >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements per row")
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        if k < 0 or k > cols:
            raise ValueError("TorchSorter.topk_rows: k = %d outside [0, last dimension = %d]" % (k, cols))
        shape = tuple(t.shape[:-1]) + (k,)
        rows = t.numel() // cols if cols else 0
        values = torch.empty(shape, dtype=t.dtype, device=t.device)
        if k == 0 or rows == 0:
            return values, torch.empty(shape, dtype=torch.int64, device=t.device)
        src = self._aligned(t)         # (the base pointer only: rows may start anywhere)
        npdt = _NP_DTYPE[t.dtype]
        idx32 = torch.empty(shape, dtype=torch.int32, device=t.device)   # uint32 columns in an int32 tensor
        self.pprims.topkRows(self.device, self._wrap(src, npdt), rows, cols, k, descending=bool(largest),
                             keysOut=self._wrap(values, npdt), indexOut=self._wrap(idx32, np.uint32))
        self.device.checkFault()
        return values, idx32.to(torch.int64) & 0xffffffff

    def _run_rows(self, what, t, descending, want_values):
        if not isinstance(t, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(t).__name__)
        if t.dtype not in _NP_DTYPE:
            raise TypeError("TorchSorter: dtype %s unsupported (int32, int64, float32, float64)" % t.dtype)
        if t.dim() < 2:
            raise ValueError("TorchSorter.%s: 2-D tensors and above, got %d dimensions (sort / argsort serve 1-D)" % (what, t.dim()))
        if t.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (t.device, self.torch_device))
        if t.numel() >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        cols = t.shape[-1]
        rows = t.numel() // cols if cols else 0
        values = torch.empty(t.shape, dtype=t.dtype, device=t.device) if want_values else None
        if rows == 0 or cols == 0:
            return values, torch.empty(t.shape, dtype=torch.int64, device=t.device)
        src = self._aligned(t)         # (the base pointer only: rows may start anywhere)
        npdt = _NP_DTYPE[t.dtype]
        idx32 = torch.empty(t.shape, dtype=torch.int32, device=t.device)   # uint32 columns in an int32 tensor
        self.pprims.sortRows(self.device, self._wrap(src, npdt), rows, cols, descending=descending,
                             keysOut=self._wrap(values, npdt) if want_values else None, indexOut=self._wrap(idx32, np.uint32))
        self.device.checkFault()
        return values, idx32.to(torch.int64) & 0xffffffff

    def sort_rows(self, t, descending=False):
        """(values, indices) like torch.sort(t, dim=-1, descending=descending, stable=True) for t.dim() >= 2: every row of the last
        dimension sorted, the leading dimensions flattened to rows; both results have t's shape, indices are int64.  A contiguous input
        is read where it lies.  It differs from torch on NaN and -0 only: floats are ordered by totalOrder, so NaNs with the sign bit
        set sort first (torch puts every NaN last) and -0 sorts before +0 (torch holds them equal).  A 1-D tensor is sort()'s."""
        return self._run_rows("sort_rows", t, bool(descending), True)

    def argsort_rows(self, t, descending=False):
        """indices like torch.argsort(t, dim=-1, descending=descending, stable=True) for t.dim() >= 2, int64, of t's shape; NaN and -0
        as in sort_rows (totalOrder).  A 1-D tensor is argsort()'s."""
        return self._run_rows("argsort_rows", t, bool(descending), False)[1]

    def _run_segments(self, what, t, offsets, descending, max_segment, global_indices, want_values):
        if not isinstance(t, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(t).__name__)
        if t.dtype not in _NP_DTYPE:
            raise TypeError("TorchSorter: dtype %s unsupported (int32, int64, float32, float64)" % t.dtype)
        if t.dim() != 1:
            raise ValueError("TorchSorter.%s: 1-D tensors only, got %d dimensions (sort_rows serves equal rows)" % (what, t.dim()))
        if not isinstance(offsets, torch.Tensor):
            raise TypeError("TorchSorter.%s: offsets must be a torch.Tensor, got %s" % (what, type(offsets).__name__))
        if offsets.dtype not in (torch.int32, torch.int64):
            raise TypeError("TorchSorter.%s: offsets must be int32 or int64, got %s" % (what, offsets.dtype))
        if offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError("TorchSorter.%s: offsets must be 1-D with num_segments + 1 entries" % what)
        n, S = t.numel(), offsets.numel() - 1
        if S == 0 and n != 0:   # (seen from the shapes alone: off[0] = 0 = off[S] cannot be t.numel())
            raise ValueError("TorchSorter.%s: offsets has one entry (no segment) for t.numel() = %d elements" % (what, n))
        if not offsets.is_cuda:   # a host tensor is checked where it lies: nothing is waited for
            if int(offsets[0]) != 0 or int(offsets[-1]) != n:
                raise ValueError("TorchSorter.%s: offsets must start at 0 and end at t.numel() = %d" % (what, n))
        self._check(t)   # (the device and the size)
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        if not offsets.is_cuda:
            if max_segment is None:
                max_segment = int((offsets[1:] - offsets[:-1]).max()) if S else 0
        elif max_segment is None:   # the one host read: first and last offset and the longest segment together
            lens = offsets[1:] - offsets[:-1]
            first, last, longest = torch.stack([offsets[0], offsets[-1], lens.max() if S else offsets[0]]).tolist()
            if first != 0 or last != n:
                raise ValueError("TorchSorter.%s: offsets must start at 0 and end at t.numel() = %d" % (what, n))
            max_segment = longest if S else 0
        max_segment = int(max_segment)
        if max_segment < 0:
            raise ValueError("TorchSorter.%s: max_segment = %d" % (what, max_segment))
        values = torch.empty(n, dtype=t.dtype, device=t.device) if want_values else None
        if n == 0 or S == 0:
            return values, torch.empty(n, dtype=torch.int64, device=t.device)
        # uint32 offsets in an int32 tensor: the low dwords of the int64 values, taken as bits (offsets from 2^31 on do not go through
        # a narrowing conversion); a new tensor
        off32 = offsets.to(device=t.device, dtype=torch.int64).contiguous().view(torch.int32)[::2].contiguous()
        if off32.data_ptr() % 16:
            off32 = off32.clone()
        src = self._aligned(t)
        npdt = _NP_DTYPE[t.dtype]
        idx32 = torch.empty(n, dtype=torch.int32, device=t.device)   # uint32 positions in an int32 tensor
        self.pprims.sortSegments(self.device, self._wrap(src, npdt), self._wrap(off32, np.uint32), S, maxSegment=max_segment,
                                 descending=descending, keysOut=self._wrap(values, npdt) if want_values else None,
                                 indexOut=self._wrap(idx32, np.uint32), globalIndex=bool(global_indices))
        self.device.checkFault()
        return values, idx32.to(torch.int64) & 0xffffffff

    def sort_segments(self, t, offsets, descending=False, max_segment=None, global_indices=False):
        """(values, indices): every segment t[offsets[s]:offsets[s + 1]] of the 1-D tensor t sorted on its own, in place of the segment
        -- per segment what torch.sort(segment, descending=descending, stable=True) returns; indices are int64 positions inside the
        segment, or in t with global_indices.  offsets: an int32 or int64 tensor of num_segments + 1 ascending entries, on the host or
        the device, the first 0 and the last t.numel(); empty segments may stand anywhere (a single entry, no segment, is accepted for
        an empty t only).  It differs from torch on NaN and -0 only:
        floats are ordered by totalOrder (sort_rows).  max_segment is an upper bound on the longest segment; up to 4096 one kernel
        sorts all segments, beyond that (or with 0, "unknown") two flat sorts do.  max_segment=None computes the longest segment,
        which for offsets on the device costs ONE host read (first and last offset are checked by the same read): the call waits for
        the stream.  With max_segment given and offsets on the device nothing reaches the host, and the ends of offsets are not
        checked (offsets that break the rules give an unspecified result, never an access outside the tensors).  A segment longer
        than a bound of 4096 or less comes back in input order."""
        return self._run_segments("sort_segments", t, offsets, bool(descending), max_segment, global_indices, True)

    def argsort_segments(self, t, offsets, descending=False, max_segment=None, global_indices=False):
        """indices of sort_segments alone, int64; NaN and -0 as there (totalOrder), the same host read for max_segment=None."""
        return self._run_segments("argsort_segments", t, offsets, bool(descending), max_segment, global_indices, False)[1]

    def _flat_input(self, t, what, one_dim):
        """the checks of topk (dtype, device, size, stream) for `what`; returns t flattened, contiguous and 16-byte aligned (a copy only
        for a strided or oddly placed input; the input is never written)"""
        if not isinstance(t, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(t).__name__)
        if t.dtype not in _NP_DTYPE:
            raise TypeError("TorchSorter: dtype %s unsupported (int32, int64, float32, float64)" % t.dtype)
        if one_dim and t.dim() != 1:
            raise ValueError("TorchSorter.%s: 1-D tensors only, got %d dimensions" % (what, t.dim()))
        if t.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (t.device, self.torch_device))
        if t.numel() >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        return self._aligned(t).reshape(-1)

    def unique(self, t, return_inverse=False, return_counts=False):
        """What torch.unique(t, sorted=True, return_inverse=..., return_counts=...) returns (dim=None): t of any number of dimensions is
        flattened; the distinct values ascending, then -- where asked -- inverse (t's shape, int64) and counts (int64).  Equal to
        torch's results on inputs without NaN and -0: keys are equal when their bits are, so -0 and +0 count as two values (-0
        first) and NaNs are grouped by bit pattern (sign bit set: first).  Like torch.unique this makes ONE host read, of the number
        of distinct values, to size the result tensors: the call waits for the stream."""
        flat = self._flat_input(t, "unique", False)
        n = flat.numel()
        if n == 0:
            out = (torch.empty(0, dtype=t.dtype, device=t.device),)
            if return_inverse:
                out += (torch.empty(t.shape, dtype=torch.int64, device=t.device),)
            if return_counts:
                out += (torch.empty(0, dtype=torch.int64, device=t.device),)
            return out if len(out) > 1 else out[0]
        npdt = _NP_DTYPE[t.dtype]
        uniq = torch.empty(n, dtype=t.dtype, device=t.device)
        count = torch.empty(1, dtype=torch.int32, device=t.device)
        inv32 = torch.empty(n, dtype=torch.int32, device=t.device) if return_inverse else None   # uint32 in int32 tensors
        cnt32 = torch.empty(n, dtype=torch.int32, device=t.device) if return_counts else None
        self.pprims.unique(self.device, self._wrap(flat, npdt), n,
                           counts=self._wrap(cnt32, np.uint32) if return_counts else False,
                           inverse=self._wrap(inv32, np.uint32) if return_inverse else False,
                           uniqueOut=self._wrap(uniq, npdt), countOut=self._wrap(count, np.uint32))
        self.device.checkFault()
        r = int(count.item()) & 0xffffffff   # the one host read
        out = (uniq[:r].clone(),)
        if return_inverse:
            out += ((inv32.to(torch.int64) & 0xffffffff).reshape(t.shape),)
        if return_counts:
            out += (cnt32[:r].to(torch.int64) & 0xffffffff,)
        return out if len(out) > 1 else out[0]

    def unique_consecutive(self, t, return_counts=False):
        """What torch.unique_consecutive(t, return_counts=...) returns for a 1-D tensor: one value per run of adjacent equal elements,
        in input order, and -- where asked -- the run lengths (int64).  Equal to torch's result on inputs without NaN and -0 (bits
        decide equality, as in unique).  Like torch.unique_consecutive this makes ONE host read, of the number of runs, to size the
        result tensors: the call waits for the stream."""
        flat = self._flat_input(t, "unique_consecutive", True)
        n = flat.numel()
        if n == 0:
            out = torch.empty(0, dtype=t.dtype, device=t.device)
            return (out, torch.empty(0, dtype=torch.int64, device=t.device)) if return_counts else out
        npdt = _NP_DTYPE[t.dtype]
        uniq = torch.empty(n, dtype=t.dtype, device=t.device)
        count = torch.empty(1, dtype=torch.int32, device=t.device)
        cnt32 = torch.empty(n, dtype=torch.int32, device=t.device) if return_counts else None
        self.pprims.runLengthEncode(self.device, self._wrap(flat, npdt), n,
                                    counts=self._wrap(cnt32, np.uint32) if return_counts else False,
                                    uniqueOut=self._wrap(uniq, npdt), countOut=self._wrap(count, np.uint32))
        self.device.checkFault()
        r = int(count.item()) & 0xffffffff   # the one host read
        if return_counts:
            return uniq[:r].clone(), cnt32[:r].to(torch.int64) & 0xffffffff
        return uniq[:r].clone()

    def _reduce(self, what, by_key, keys, values, op, descending, return_counts):
        if op not in ("sum", "min", "max"):
            raise ValueError("TorchSorter.%s: op must be 'sum', 'min' or 'max', got %r" % (what, op))
        k = self._flat_input(keys, what, True)
        v = self._flat_input(values, what, True)
        n = k.numel()
        if v.numel() != n:
            raise ValueError("TorchSorter.%s: %d keys but %d values" % (what, n, v.numel()))
        if n == 0:
            out = (torch.empty(0, dtype=keys.dtype, device=keys.device), torch.empty(0, dtype=values.dtype, device=keys.device))
            return out + (torch.empty(0, dtype=torch.int64, device=keys.device),) if return_counts else out
        kdt, vdt = _NP_DTYPE[keys.dtype], _NP_DTYPE[values.dtype]
        uniq = torch.empty(n, dtype=keys.dtype, device=keys.device)
        red = torch.empty(n, dtype=values.dtype, device=keys.device)
        count = torch.empty(1, dtype=torch.int32, device=keys.device)
        cnt32 = torch.empty(n, dtype=torch.int32, device=keys.device) if return_counts else None   # uint32 in an int32 tensor
        args = dict(op=op, counts=self._wrap(cnt32, np.uint32) if return_counts else False, uniqueOut=self._wrap(uniq, kdt),
                    reducedOut=self._wrap(red, vdt), countOut=self._wrap(count, np.uint32))
        if by_key:
            self.pprims.reduceByKey(self.device, self._wrap(k, kdt), self._wrap(v, vdt), n, descending=bool(descending), **args)
        else:
            self.pprims.reduceRuns(self.device, self._wrap(k, kdt), self._wrap(v, vdt), n, **args)
        self.device.checkFault()
        r = int(count.item()) & 0xffffffff   # the one host read
        out = (uniq[:r].clone(), red[:r].clone())
        return out + (cnt32[:r].to(torch.int64) & 0xffffffff,) if return_counts else out

    def reduce_by_key(self, keys, values, op="sum", descending=False, return_counts=False):
        """(unique_keys, reduced[, counts]): the distinct keys in sorted order (descending: largest first) and `op` ("sum", "min",
        "max") over the values of each -- torch.unique(keys, return_inverse=True) followed by index_add_ / scatter_reduce_ -- and,
        where asked, how often each key occurs (int64).  keys and values: 1-D tensors of the same length on the sorter's device,
        int32 / int64 / float32 / float64 each, in any combination; reduced has the values' dtype.  Keys are equal when their bits
        are (as in unique).  Integer sums wrap; float sums are IEEE adds in an unspecified association, the same bits on every call
        (index_add_'s atomics are not).  min / max are taken in IEEE totalOrder, -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN:
        a NaN is the minimum or the maximum by its sign, NOT propagated as torch's amin / amax do, and -0 is below +0; without NaN
        they give amin / amax.  Like unique this makes ONE host read, of the number of keys: the call waits for the stream."""
        return self._reduce("reduce_by_key", True, keys, values, op, descending, return_counts)

    def reduce_consecutive(self, keys, values, op="sum", return_counts=False):
        """reduce_by_key for keys that are already grouped: one (key, reduced[, count]) per run of adjacent keys with identical bits,
        in input order -- the runs of unique_consecutive.  The same types, operators (min / max in totalOrder) and host read."""
        return self._reduce("reduce_consecutive", False, keys, values, op, False, return_counts)

    def _scan(self, what, keys, values, op, exclusive, init):
        if op not in ("sum", "min", "max"):
            raise ValueError("TorchSorter.%s: op must be 'sum', 'min' or 'max', got %r" % (what, op))
        if init is not None and not exclusive:
            raise ValueError("TorchSorter.%s: an inclusive scan takes no init" % what)
        k = self._flat_input(keys, what, True) if keys is not None else None
        v = self._flat_input(values, what, True)
        n = v.numel()
        if k is not None and k.numel() != n:
            raise ValueError("TorchSorter.%s: %d keys but %d values" % (what, k.numel(), n))
        out = torch.empty(n, dtype=values.dtype, device=values.device)
        if n == 0:
            return out
        vdt = _NP_DTYPE[values.dtype]
        if k is None:
            self.pprims.scanTyped(self.device, self._wrap(out, vdt), self._wrap(v, vdt), n, op=op, exclusive=bool(exclusive), init=init)
        else:
            self.pprims.scanByKey(self.device, self._wrap(k, _NP_DTYPE[keys.dtype]), self._wrap(out, vdt), self._wrap(v, vdt), n, op=op,
                                  exclusive=bool(exclusive), init=init)
        self.device.checkFault()
        return out

    def cumsum(self, t):
        """torch.cumsum(t, 0, dtype=t.dtype) for a 1-D tensor of int32 / int64 / float32 / float64.  The result has the INPUT's dtype:
        int32 sums wrap in 32 bits, unlike torch.cumsum(t, 0), which promotes int32 to int64.  Float sums are IEEE adds in an
        unspecified association, the same bits on every call (torch.cumsum makes no such promise).  No host read."""
        return self._scan("cumsum", None, t, "sum", False, None)

    def cummax(self, t):
        """The VALUES of torch.cummax(t, 0) for a 1-D tensor; no indices.  The maximum is taken in IEEE totalOrder, -NaN < -inf < ...
        < -0 < +0 < ... < +inf < +NaN: a NaN is the largest or the smallest element by its sign and is NOT propagated as torch's
        cummax does, and -0 is below +0; without NaN the values are torch's."""
        return self._scan("cummax", None, t, "max", False, None)

    def cummin(self, t):
        """The VALUES of torch.cummin(t, 0) for a 1-D tensor; no indices.  totalOrder, not torch's NaN propagation, as cummax."""
        return self._scan("cummin", None, t, "min", False, None)

    def scan_by_key(self, keys, values, op="sum", exclusive=False, init=None):
        """The scan of `values` within every run of adjacent keys with identical bits (the runs of unique_consecutive): thrust's
        inclusive_scan_by_key / exclusive_scan_by_key, which torch does not have.  keys and values: 1-D tensors of the same length,
        int32 / int64 / float32 / float64 each, in any combination; the result has the values' dtype (int32 sums wrap).  op "sum",
        "min" or "max" (totalOrder, as cummax).  exclusive: a run's first element gets init -- without one the operator's identity
        pattern: 0, the type's largest pattern in that order for "min", its smallest for "max" --, every other one op(init, the
        inclusive result in front of it).  An inclusive scan takes no init.  No host read."""
        return self._scan("scan_by_key", keys, values, op, exclusive, init)

    def _flat_mask(self, mask, what):
        """the checks of _flat_input for a bool / uint8 mask; returns it flattened, contiguous and 16-byte aligned"""
        if not isinstance(mask, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(mask).__name__)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError("TorchSorter.%s: the mask must be bool or uint8, got %s" % (what, mask.dtype))
        if mask.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (mask.device, self.torch_device))
        if mask.numel() >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        return self._aligned(mask).reshape(-1)

    def _compact_flagged(self, what, t, mask, partition, want_index):
        """(items or None, int64 positions or None, S) of the flagged compaction of t (None: positions only) by mask"""
        m = self._flat_mask(mask, what)
        flat = None
        if t is not None:
            flat = self._flat_input(t, what, False)
            if tuple(t.shape) != tuple(mask.shape):
                raise ValueError("TorchSorter.%s: the mask's shape %s is not the tensor's %s (no broadcasting)"
                                 % (what, tuple(mask.shape), tuple(t.shape)))
        n = m.numel()
        dev = mask.device
        if n == 0:
            return (torch.empty(0, dtype=t.dtype, device=dev) if t is not None else None,
                    torch.empty(0, dtype=torch.int64, device=dev) if want_index else None, 0)
        out = torch.empty(n, dtype=t.dtype, device=dev) if t is not None else None
        idx32 = torch.empty(n, dtype=torch.int32, device=dev) if want_index else None   # uint32 positions in an int32 tensor
        count = torch.empty(1, dtype=torch.int32, device=dev)
        self.pprims.compactFlagged(self.device, self._wrap(m, np.uint8), n,
                                   items=self._wrap(flat, _NP_DTYPE[t.dtype]) if t is not None else None, partition=partition,
                                   itemsOut=self._wrap(out, _NP_DTYPE[t.dtype]) if t is not None else None,
                                   indexOut=self._wrap(idx32, np.uint32) if want_index else None, countOut=self._wrap(count, np.uint32))
        self.device.checkFault()
        s = int(count.item()) & 0xffffffff   # the one host read
        keep = n if partition else s
        if out is not None and not partition:
            out = out[:s].clone()
        return out, (idx32[:keep].to(torch.int64) & 0xffffffff) if want_index else None, s

    def masked_select(self, t, mask):
        """torch.masked_select(t, mask) for a mask of t's shape (NO broadcasting), bool or uint8 (any non-zero byte selects): the
        selected elements of t in row-major order, 1-D, bit for bit.  t: int32 / int64 / float32 / float64, any number of dimensions.
        Like torch.masked_select this makes ONE host read, of the number of selected elements: the call waits for the stream."""
        return self._compact_flagged("masked_select", t, mask, False, False)[0]

    def nonzero(self, mask):
        """torch.nonzero(mask) for a bool or uint8 mask of any number of dimensions: int64 of shape [S, mask.dim()], the positions of
        the non-zero elements in row-major order (the flat positions come from the device, they are unravelled with torch ops).
        ONE host read, as torch.nonzero makes."""
        idx = self._compact_flagged("nonzero", None, mask, False, True)[1]
        if idx.numel() == 0:
            return torch.empty((0, mask.dim()), dtype=torch.int64, device=mask.device)
        cols = []
        for size in reversed(mask.shape):
            cols.append(idx % size)
            idx = idx // size
        return torch.stack(cols[::-1], dim=1)

    def partition(self, t, mask):
        """(out, S): out has t's elements flattened -- first the S elements whose mask byte is non-zero, then the others, both in
        input (row-major) order: thrust's stable_partition with a stencil.  mask as in masked_select.  ONE host read, of S."""
        out, _, s = self._compact_flagged("partition", t, mask, True, False)
        return out, s

    def select_if(self, t, cmp, threshold, values=None, return_indices=False):
        """t[t cmp threshold] for a 1-D tensor; cmp is "lt", "le", "gt", "ge", "eq" or "ne" (or "<", "<=", ">", ">=", "==", "!=").
        Returns the selected elements in input order, then -- where given / asked -- values[t cmp threshold] (a 1-D tensor of t's
        length, int32 / int64 / float32 / float64 whatever t's dtype) and their int64 positions; one tensor or a tuple.
        The comparison is the order of sort(): integers by value, floats by IEEE totalOrder.  It differs from torch's t[t < x] on
        NaN and -0 ONLY: NaNs are ordered by sign and payload (-NaN below -inf, +NaN above +inf) where torch's comparisons with a
        NaN are all false (and != true), -0 is below +0 where torch holds them equal, and "eq" / "ne" compare bits (so a NaN equals
        itself).  Inputs and thresholds without NaN and -0 give torch's result bit for bit.  ONE host read, of the number selected."""
        if cmp not in ("lt", "le", "gt", "ge", "eq", "ne", "<", "<=", ">", ">=", "==", "!="):
            raise ValueError("TorchSorter.select_if: cmp must be 'lt', 'le', 'gt', 'ge', 'eq' or 'ne', got %r" % (cmp,))
        k = self._flat_input(t, "select_if", True)
        v = self._flat_input(values, "select_if", True) if values is not None else None
        n = k.numel()
        if v is not None and v.numel() != n:
            raise ValueError("TorchSorter.select_if: %d elements but %d values" % (n, v.numel()))
        dev = t.device
        if n == 0:
            out = (torch.empty(0, dtype=t.dtype, device=dev),)
            if v is not None:
                out += (torch.empty(0, dtype=values.dtype, device=dev),)
            if return_indices:
                out += (torch.empty(0, dtype=torch.int64, device=dev),)
            return out if len(out) > 1 else out[0]
        kdt = _NP_DTYPE[t.dtype]
        kout = torch.empty(n, dtype=t.dtype, device=dev)
        vout = torch.empty(n, dtype=values.dtype, device=dev) if v is not None else None
        idx32 = torch.empty(n, dtype=torch.int32, device=dev) if return_indices else None   # uint32 positions in an int32 tensor
        count = torch.empty(1, dtype=torch.int32, device=dev)
        if isinstance(threshold, torch.Tensor):
            threshold = threshold.item()
        self.pprims.compactIf(self.device, self._wrap(k, kdt), n, cmp, threshold,
                              values=self._wrap(v, _NP_DTYPE[values.dtype]) if v is not None else None,
                              keysOut=self._wrap(kout, kdt),
                              valuesOut=self._wrap(vout, _NP_DTYPE[values.dtype]) if v is not None else None,
                              indexOut=self._wrap(idx32, np.uint32) if return_indices else None, countOut=self._wrap(count, np.uint32))
        self.device.checkFault()
        s = int(count.item()) & 0xffffffff   # the one host read
        out = (kout[:s].clone(),)
        if v is not None:
            out += (vout[:s].clone(),)
        if return_indices:
            out += (idx32[:s].to(torch.int64) & 0xffffffff,)
        return out if len(out) > 1 else out[0]

    def _counts(self, buf_call, num_bins, dev):
        """int64 counts of num_bins bins from a call that fills a uint32 Buffer over an int32 tensor"""
        c32 = torch.empty(num_bins, dtype=torch.int32, device=dev)   # uint32 counters in an int32 tensor
        buf_call(self._wrap(c32, np.uint32))
        self.device.checkFault()
        return c32.to(torch.int64) & 0xffffffff

    def bincount(self, t, num_bins=None):
        """torch.bincount(t) for a 1-D int32 / int64 tensor: int64 counts, counts[v] = the elements equal to v for 0 <= v < num_bins.
        num_bins omitted: max(t) + 1, as torch sizes its result -- computing it costs ONE host read, as it does in torch; with
        num_bins given nothing reaches the host, the result always has num_bins elements, and elements >= num_bins are ignored
        (torch's minlength only ever lengthens).  Negative elements are ignored where torch raises; a tensor of nothing but negative
        elements gives an empty result.  Weights are not offered: for
        sums of a second column per key use reduce_by_key, whose float sums are reproducible bit for bit."""
        k = self._flat_input(t, "bincount", True)
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("TorchSorter.bincount: integer tensors only (int32, int64), got %s" % t.dtype)
        n = k.numel()
        if num_bins is None:
            num_bins = max(int(k.max().item()) + 1, 0) if n else 0   # the one host read; nothing but negative elements: no bins
        num_bins = int(num_bins)
        if num_bins < 0 or num_bins >= 1 << 31:
            raise ValueError("TorchSorter.bincount: num_bins = %d outside [0, 2^31)" % num_bins)
        if num_bins == 0:
            return torch.empty(0, dtype=torch.int64, device=t.device)
        kdt = _NP_DTYPE[t.dtype]
        return self._counts(lambda c: self.pprims.binCount(self.device, self._wrap(k, kdt), n, num_bins, countsOut=c), num_bins, t.device)

    def histogram(self, t, edges):
        """numpy.histogram(t, bins=edges)[0] for a 1-D tensor t and a 1-D tensor `edges` of the same dtype and device with 2 .. 4097
        non-decreasing elements: int64 counts of the len(edges) - 1 bins [edges[b], edges[b + 1]), the last one closed.  Equal to
        numpy on input without NaN: the comparisons are those of sort() -- integers by value, floats by IEEE totalOrder on bits, so
        -0 is below +0 (an edge of +0 leaves -0 outside) and NaNs lie beyond the infinities, outside any finite edges.  Nothing
        reaches the host."""
        k = self._flat_input(t, "histogram", True)
        e = self._flat_input(edges, "histogram", True)
        if e.dtype != t.dtype:
            raise TypeError("TorchSorter.histogram: edges are %s, the tensor %s" % (e.dtype, t.dtype))
        bins = e.numel() - 1
        if bins < 1 or bins > 4096:
            raise ValueError("TorchSorter.histogram: %d edges; 2 .. 4097 (1 .. 4096 bins)" % e.numel())
        kdt = _NP_DTYPE[t.dtype]
        return self._counts(lambda c: self.pprims.histogramRange(self.device, self._wrap(k, kdt), k.numel(), self._wrap(e, kdt), bins,
                                                                 include_upper=True, countsOut=c), bins, t.device)

    def histc(self, t, bins=100, min=0, max=0):
        """Counts of `bins` equal-width bins between min and max, int64: the edges are torch.linspace(min, max, bins + 1) computed in
        float64 on the CPU and cast to t's dtype, and the result equals numpy.histogram on those edges EXACTLY (histogram() above; the last bin
        is closed, elements outside [min, max] are ignored).  torch.histc computes each element's bin by a division instead; for an
        element within a rounding error of an edge the two can differ by one bin.  min == max (the default): the tensor's own
        minimum and maximum, which costs one host read; if those are equal too, min - 1 and max + 1, as torch does.  For an integer
        tensor the cast truncates the edges towards zero: the bins are then of unequal width, and edges that fall on one integer
        give empty bins -- still numpy.histogram on those integer edges."""
        k = self._flat_input(t, "histc", True)
        bins = int(bins)
        if bins < 1 or bins > 4096:
            raise ValueError("TorchSorter.histc: bins = %d outside [1, 4096]" % bins)
        lo, hi = float(min), float(max)
        if lo > hi:
            raise ValueError("TorchSorter.histc: max must be larger than min")
        if lo == hi and k.numel():
            lo, hi = float(k.min().item()), float(k.max().item())
        if lo == hi:
            lo, hi = lo - 1.0, hi + 1.0
        edges = torch.linspace(lo, hi, bins + 1, dtype=torch.float64).to(t.dtype).to(t.device)   # (on the CPU: the same edges everywhere)
        return self.histogram(k, edges)

    def _merge_input(self, t, what):
        """the checks of _flat_input for a 1-D input of merge(); contiguous, but at ANY element offset: the merge takes its inputs
        at their element's alignment, so a view such as t[1:] goes through without a copy (a strided one is copied)"""
        if not isinstance(t, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(t).__name__)
        if t.dtype not in _NP_DTYPE:
            raise TypeError("TorchSorter: dtype %s unsupported (int32, int64, float32, float64)" % t.dtype)
        if t.dim() != 1:
            raise ValueError("TorchSorter.%s: 1-D tensors only, got %d dimensions" % (what, t.dim()))
        if t.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (t.device, self.torch_device))
        return t.contiguous()

    def merge(self, a, b, descending=False, values=None, return_indices=False):
        """What torch.sort(torch.cat((a, b)), descending=descending, stable=True) returns for 1-D tensors a and b of one dtype that
        are each sorted that way already -- by one merge instead of a sort: the merged values, then -- where given -- the merged
        `values` (a pair of 1-D tensors of a's and b's lengths and one dtype, int32 / int64 / float32 / float64 whatever the keys'),
        then -- where asked -- the int64 indices into the concatenation; one tensor or a tuple.  Equal elements keep the order of the
        concatenation: a's before b's.  The order is that of sort(): floats by totalOrder, so inputs must be sorted with -0 before
        +0 and NaNs by sign at the two ends; without NaN and -0 that is torch's order.  Inputs that are not sorted give an output
        in unspecified order.  Contiguous views at any element offset are read where they lie, without a copy.  Nothing reaches
        the host."""
        ka, kb = self._merge_input(a, "merge"), self._merge_input(b, "merge")
        if ka.dtype != kb.dtype:
            raise TypeError("TorchSorter.merge: a is %s, b %s" % (ka.dtype, kb.dtype))
        va = vb = None
        if values is not None:
            if not isinstance(values, (tuple, list)) or len(values) != 2:
                raise ValueError("TorchSorter.merge: values is a pair (values of a, values of b)")
            va, vb = self._merge_input(values[0], "merge"), self._merge_input(values[1], "merge")
            if va.dtype != vb.dtype:
                raise TypeError("TorchSorter.merge: the values are %s and %s" % (va.dtype, vb.dtype))
            if va.numel() != ka.numel() or vb.numel() != kb.numel():
                raise ValueError("TorchSorter.merge: %d and %d elements but %d and %d values" % (ka.numel(), kb.numel(), va.numel(), vb.numel()))
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        na, nb = ka.numel(), kb.numel()
        n = na + nb
        if n >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")
        dev = ka.device
        kout = torch.empty(n, dtype=ka.dtype, device=dev)
        vout = torch.empty(n, dtype=va.dtype, device=dev) if va is not None else None
        idx32 = torch.empty(n, dtype=torch.int32, device=dev) if return_indices else None   # uint32 positions in an int32 tensor
        if n:
            kdt = _NP_DTYPE[ka.dtype]
            if va is not None:
                vdt = _NP_DTYPE[va.dtype]
                self.pprims.mergePairs(self.device, self._wrap(ka, kdt), self._wrap(va, vdt), self._wrap(kb, kdt), self._wrap(vb, vdt),
                                       self._wrap(kout, kdt), self._wrap(vout, vdt), na, nb, descending=bool(descending),
                                       indexOut=self._wrap(idx32, np.uint32) if return_indices else None)
            else:
                self.pprims.mergeKeys(self.device, self._wrap(ka, kdt), self._wrap(kb, kdt), self._wrap(kout, kdt), na, nb,
                                      descending=bool(descending), indexOut=self._wrap(idx32, np.uint32) if return_indices else None)
            self.device.checkFault()
        out = (kout,)
        if va is not None:
            out += (vout,)
        if return_indices:
            out += (idx32.to(torch.int64) & 0xffffffff,)
        return out if len(out) > 1 else out[0]

    def _set_op(self, op, what, a, b, descending, values, return_indices):
        ka, kb = self._merge_input(a, what), self._merge_input(b, what)
        if ka.dtype != kb.dtype:
            raise TypeError("TorchSorter.%s: a is %s, b %s" % (what, ka.dtype, kb.dtype))
        va = vb = None
        if values is not None:
            if not isinstance(values, (tuple, list)) or len(values) != 2:
                raise ValueError("TorchSorter.%s: values is a pair (values of a, values of b)" % what)
            va, vb = self._merge_input(values[0], what), self._merge_input(values[1], what)
            if va.dtype != vb.dtype:
                raise TypeError("TorchSorter.%s: the values are %s and %s" % (what, va.dtype, vb.dtype))
            if va.numel() != ka.numel() or vb.numel() != kb.numel():
                raise ValueError("TorchSorter.%s: %d and %d elements but %d and %d values" % (what, ka.numel(), kb.numel(), va.numel(), vb.numel()))
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        na, nb = ka.numel(), kb.numel()
        if na + nb >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")
        cap = na + nb if op in ("union", "symmetric_difference") else na
        dev = ka.device
        kout = torch.empty(cap, dtype=ka.dtype, device=dev)
        vout = torch.empty(cap, dtype=va.dtype, device=dev) if va is not None else None
        idx32 = torch.empty(cap, dtype=torch.int32, device=dev) if return_indices else None   # uint32 positions in an int32 tensor
        s = 0
        if cap:
            count = torch.empty(1, dtype=torch.int32, device=dev)
            kdt = _NP_DTYPE[ka.dtype]
            vdt = _NP_DTYPE[va.dtype] if va is not None else None
            self.pprims.setOp(self.device, op, self._wrap(ka, kdt), self._wrap(kb, kdt), self._wrap(kout, kdt), na, nb,
                              descending=bool(descending), valuesA=self._wrap(va, vdt) if va is not None else None,
                              valuesB=self._wrap(vb, vdt) if va is not None else None,
                              valuesOut=self._wrap(vout, vdt) if va is not None else None,
                              indexOut=self._wrap(idx32, np.uint32) if return_indices else None, countOut=self._wrap(count, np.uint32))
            self.device.checkFault()
            s = int(count.item()) & 0xffffffff   # the one host read
        out = (kout[:s].clone(),)
        if va is not None:
            out += (vout[:s].clone(),)
        if return_indices:
            out += (idx32[:s].to(torch.int64) & 0xffffffff,)
        return out if len(out) > 1 else out[0]

    def intersect(self, a, b, descending=False, values=None, return_indices=False):
        """The elements of the sorted 1-D tensor a that the sorted 1-D tensor b of the same dtype holds too: for inputs without
        duplicates, NaN or -0 what numpy.intersect1d(a, b, assume_unique=True) returns (descending=True: in descending order).
        With duplicates the semantics are thrust's set_intersection: of an element that occurs m times in a and n times in b the
        first min(m, n) of a's.  Elements are equal when their bits are; the order is that of merge().  Returns the result, then --
        where given -- the kept elements' own `values` (a pair of 1-D tensors of a's and b's lengths and one dtype), then -- where
        asked -- their int64 indices into torch.cat((a, b)); one tensor or a tuple.  Contiguous views at any element offset are read
        where they lie.  ONE host read, of the size of the result."""
        return self._set_op("intersection", "intersect", a, b, descending, values, return_indices)

    def union(self, a, b, descending=False, values=None, return_indices=False):
        """numpy.union1d(a, b) of sorted 1-D tensors without duplicates; with duplicates thrust's set_union: max(m, n) copies, all
        of a's and then the last n - m of b's.  Everything else as intersect()."""
        return self._set_op("union", "union", a, b, descending, values, return_indices)

    def difference(self, a, b, descending=False, values=None, return_indices=False):
        """numpy.setdiff1d(a, b, assume_unique=True) of sorted 1-D tensors without duplicates; with duplicates thrust's
        set_difference: the last max(m - n, 0) of a's copies.  Everything else as intersect()."""
        return self._set_op("difference", "difference", a, b, descending, values, return_indices)

    def symmetric_difference(self, a, b, descending=False, values=None, return_indices=False):
        """numpy.setxor1d(a, b, assume_unique=True) of sorted 1-D tensors without duplicates; with duplicates thrust's
        set_symmetric_difference: |m - n| copies, the last of a's or of b's.  Everything else as intersect()."""
        return self._set_op("symmetric_difference", "symmetric_difference", a, b, descending, values, return_indices)

    def join(self, a, b, how="inner", descending=False):
        """The join of the sorted 1-D tensors a and b of one dtype, as int64 positions (index_a, index_b): every pair (i, j) with
        a[i] equal to b[j] -- all m x n pairs of an element that occurs m times in a and n times in b, where intersect() keeps
        min(m, n) elements -- ordered by i, then by j.  how="left" also keeps every a[i] without a match, once, with index_b -1;
        how="semi" returns index_a alone, every i with a match once; how="anti" index_a alone, every i without one.  Elements are
        equal when their bits are; the order the inputs must be sorted in is that of merge().  Inputs that are not sorted give
        unspecified rows, never a position outside a and b.  Contiguous views at any element offset are read where they lie.  It
        makes a counting call, ONE host read of the 8-byte row count, then the filling call; it raises ValueError when the rows
        plus the elements of a exceed 0xFFF00000."""
        from .pprims import JOIN_KINDS, JOIN_MAX_ELEMS
        if how not in JOIN_KINDS:
            raise ValueError("TorchSorter.join: how must be 'inner', 'left', 'semi' or 'anti', got %r" % (how,))
        ka, kb = self._merge_input(a, "join"), self._merge_input(b, "join")
        if ka.dtype != kb.dtype:
            raise TypeError("TorchSorter.join: a is %s, b %s" % (ka.dtype, kb.dtype))
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        na, nb = ka.numel(), kb.numel()
        if na + nb > JOIN_MAX_ELEMS:
            raise ValueError("TorchSorter.join: at most %d elements" % JOIN_MAX_ELEMS)
        dev = ka.device
        pairs = how in ("inner", "left")
        total = 0
        kdt = _NP_DTYPE[ka.dtype]
        wa, wb = self._wrap(ka, kdt), self._wrap(kb, kdt)
        if na:
            count = torch.empty(1, dtype=torch.int64, device=dev)
            self.pprims.joinSorted(self.device, how, wa, wb, na, nb, countOut=self._wrap(count, np.uint64), descending=bool(descending))
            self.device.checkFault()
            total = int(count.item())   # the one host read
            if na + total > JOIN_MAX_ELEMS:
                raise ValueError("TorchSorter.join: %d rows; the rows and the %d elements of a are at most %d together" % (total, na, JOIN_MAX_ELEMS))
        ia32 = torch.empty(total, dtype=torch.int32, device=dev)   # uint32 positions in int32 tensors
        ib32 = torch.empty(total, dtype=torch.int32, device=dev) if pairs else None
        if total:
            self.pprims.joinSorted(self.device, how, wa, wb, na, nb, cap=total, indexA=self._wrap(ia32, np.uint32),
                                   indexB=self._wrap(ib32, np.uint32) if pairs else None, countOut=self._wrap(count, np.uint64),
                                   descending=bool(descending))
            self.device.checkFault()
        ia = ia32.to(torch.int64) & 0xffffffff
        if not pairs:
            return ia
        ib = ib32.to(torch.int64)
        return ia, torch.where(ib == -1, ib, ib & 0xffffffff)   # ADLHIP_JOIN_NONE is -1 as an int32

    def repeat_interleave(self, values, repeats, output_size=None):
        """What torch.repeat_interleave(values, repeats, output_size=output_size) returns for a 1-D `values` of 4 or 8 bytes per
        element and a 1-D integer tensor `repeats` of the same length (or of one element, or a Python int, for all of them):
        values[i] repeated repeats[i] times, in order.  The repeats are non-negative and below 2^32, and their number plus their sum
        is at most 0xFFF00000.  With output_size given -- it must be the sum of the repeats, as torch asks; that is not checked, and
        elements behind the sum are left unwritten -- nothing reaches the host; without it there is a counting call and one host read
        of the 8-byte sum.  Contiguous views at any element offset are read where they lie."""
        from .pprims import JOIN_MAX_ELEMS
        if not isinstance(values, torch.Tensor):
            raise TypeError("TorchSorter: expected a torch.Tensor, got %s" % type(values).__name__)
        if values.dim() != 1 or values.element_size() not in (4, 8) or values.is_complex():
            raise TypeError("TorchSorter.repeat_interleave: values is 1-D with 4 or 8 bytes per element, got %s with %d dimensions"
                            % (values.dtype, values.dim()))
        if values.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (values.device, self.torch_device))
        n = values.numel()
        if isinstance(repeats, int) and not isinstance(repeats, bool):
            repeats = torch.full((1,), repeats, dtype=torch.int64, device=values.device)
        if not isinstance(repeats, torch.Tensor) or repeats.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise TypeError("TorchSorter.repeat_interleave: repeats is an integer tensor or a Python int")
        if repeats.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (repeats.device, self.torch_device))
        if repeats.dim() > 1 or repeats.numel() not in (1, n):
            raise ValueError("TorchSorter.repeat_interleave: repeats has one element or one per element of values")
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        counts = repeats.reshape(-1).expand(n).to(torch.int32).contiguous()   # uint32 counts in an int32 tensor
        src = values.contiguous()
        vdt = np.uint32 if values.element_size() == 4 else np.uint64
        dev = values.device
        wc, wv = self._wrap(counts, np.uint32), self._wrap(src, vdt)
        if output_size is None:
            total = 0
            if n:
                count = torch.empty(1, dtype=torch.int64, device=dev)
                self.pprims.expandRuns(self.device, wc, n, countOut=self._wrap(count, np.uint64))
                self.device.checkFault()
                total = int(count.item())   # the one host read
        else:
            total = int(output_size)
            if total < 0:
                raise ValueError("TorchSorter.repeat_interleave: output_size is negative")
        if n + total > JOIN_MAX_ELEMS:
            raise ValueError("TorchSorter.repeat_interleave: %d elements from %d; at most %d together" % (total, n, JOIN_MAX_ELEMS))
        out = torch.empty(total, dtype=values.dtype, device=dev)
        if total and n:
            count = torch.empty(1, dtype=torch.int64, device=dev)
            self.pprims.expandRuns(self.device, wc, n, cap=total, values=wv, valuesOut=self._wrap(out, vdt), countOut=self._wrap(count, np.uint64))
            self.device.checkFault()
        return out

    def searchsorted(self, sorted_sequence, values, right=False, side=None, out_int32=False, descending=False):
        """What torch.searchsorted(sorted_sequence, values, right=right, side=side, out_int32=out_int32) returns for a 1-D
        `sorted_sequence`: for every element of `values` -- a tensor of any shape and the same dtype, or a Python scalar -- the index
        in front of which it would be inserted to keep the sequence sorted: in front of its equals (left, the default) or behind
        them (right=True or side="right").  The result has the shape of `values` and is int64, or int32 with out_int32.
        `sorted_sequence` is contiguous at any element offset (t[1:] is searched where it lies, a strided view is copied) and sorted
        ascending, or descending with descending=True (which torch does not offer).  It differs from torch only on -0 against +0
        and on NaN: the order is that of sort(), floats by totalOrder, so the sequence must be sorted with -0 before +0 and NaNs by
        sign at the two ends, -0 is searched as a value below +0, and a NaN needle finds the NaNs of its own sign and payload.
        A sequence that is not sorted gives unspecified indices in [0, len].  Not offered: `sorter=` and a batched N-D
        `sorted_sequence`; for those the caller sorts first, or loops over the rows.  Nothing reaches the host."""
        seq = self._merge_input(sorted_sequence, "searchsorted")
        if side is not None:
            if side not in ("left", "right"):
                raise ValueError("TorchSorter.searchsorted: side must be 'left' or 'right', got %r" % (side,))
            if side == "left" and right:
                raise ValueError("TorchSorter.searchsorted: side is 'left' but right is True")
            right = side == "right"
        if not isinstance(values, torch.Tensor):
            if isinstance(values, (bool, str)) or not isinstance(values, (int, float)):
                raise TypeError("TorchSorter.searchsorted: values is a tensor or a Python number, got %s" % type(values).__name__)
            values = torch.tensor(values, dtype=seq.dtype, device=seq.device)
        if values.dtype != seq.dtype:
            raise TypeError("TorchSorter.searchsorted: sorted_sequence is %s, values %s" % (seq.dtype, values.dtype))
        if values.device != self.torch_device:
            raise ValueError("TorchSorter: tensor is on %s, the sorter on %s" % (values.device, self.torch_device))
        if torch.cuda.current_stream(self.torch_device).cuda_stream != self.raw_stream:
            raise RuntimeError("TorchSorter: bound to the stream that was current at construction; another stream is current now")
        m, n = seq.numel(), values.numel()
        if m >= 1 << 32 or n >= 1 << 32:
            raise ValueError("TorchSorter: fewer than 2^32 elements")
        pos32 = torch.empty(n, dtype=torch.int32, device=seq.device)   # uint32 positions in an int32 tensor
        if n:
            needles = self._aligned(values.contiguous().view(-1))
            kdt = _NP_DTYPE[seq.dtype]
            self.pprims.searchSorted(self.device, self._wrap(seq, kdt), self._wrap(needles, kdt), self._wrap(pos32, np.uint32), m, n,
                                     descending=bool(descending), right=bool(right))
            self.device.checkFault()
        out = pos32 if out_int32 else pos32.to(torch.int64) & 0xffffffff
        return out.view(values.shape)

    def bucketize(self, input, boundaries, right=False, out_int32=False):
        """What torch.bucketize(input, boundaries, right=right, out_int32=out_int32) returns: searchsorted(boundaries, input) -- for
        every element of `input` (any shape, or a Python scalar) the index of its bucket among the 1-D sorted `boundaries`: with
        right=False boundaries[i - 1] < x <= boundaries[i], with right=True boundaries[i - 1] <= x < boundaries[i].  Everything else,
        the difference from torch on -0 and NaN included, as searchsorted()."""
        return self.searchsorted(boundaries, input, right=right, out_int32=out_int32)

    def sort(self, t, descending=False):
        """(values, indices) like torch.sort(t, descending=descending, stable=True); indices are int64."""
        return self._run(t, bool(descending), True)

    def argsort(self, t, descending=False):
        """indices like torch.argsort(t, descending=descending, stable=True), int64."""
        return self._run(t, bool(descending), False)[1]
