"""Host-side driver of libbyzagg: one `Engine` per GPU.

The engine accepts either
  * host matrices (C-contiguous np.float32, exactly what reference server.py:34-35 allocates): staged to
    the device by the library, results come back as numpy -- this is the drop-in path; or
  * device-resident matrices (torch CUDA tensors, or `DeviceBuffer`s allocated through the library):
    nothing crosses PCIe, work is queued on the caller's current stream -- this is the path the large
    configurations and bench.py use.
There is no CPU implementation behind it: every method ends in a HIP kernel or raises.
"""
import ctypes
import itertools
import os

import numpy as np

from . import _native

NAME_TO_ID = {'NoDefense': 0, 'Krum': 1, 'TrimmedMean': 2, 'Bulyan': 3}


def dnc_columns(n_cols, sub_dim, n_iters=1, seed=0):
    """DnC's column samples, drawn on the host so that the library stays deterministic: an (n_iters, min(sub_dim, n_cols))
    int64 array, every row np.sort(rng.choice(n_cols, sub_dim, replace=False)) from ONE np.random.default_rng(seed), or
    arange(n_cols) when sub_dim >= n_cols."""
    n_cols, sub_dim, n_iters = int(n_cols), int(sub_dim), int(n_iters)
    if n_iters < 1 or sub_dim < 1 or n_cols < 1:
        raise ValueError('dnc_columns: n_iters, sub_dim and n_cols must be >= 1')
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_iters):
        if sub_dim >= n_cols:
            rows.append(np.arange(n_cols, dtype=np.int64))
        else:
            rows.append(np.sort(rng.choice(n_cols, sub_dim, replace=False)).astype(np.int64))
    return np.stack(rows)


def signguard_window(n_cols, frac=0.1, seed=0):
    """SignGuard's census window, drawn on the host so that the library stays deterministic: (c0, m) with
    m = max(1, int(frac * n_cols)) and c0 = np.random.default_rng(seed).integers(0, n_cols - m + 1), i.e. uniform in
    [0, n_cols - m] with BOTH ends included.  The authors' code draws its start with an exclusive upper end and so cannot
    express frac = 1; here frac = 1 is the whole row."""
    n_cols, frac = int(n_cols), float(frac)
    if n_cols < 1 or not 0.0 < frac <= 1.0:
        raise ValueError('signguard_window: n_cols must be >= 1 and 0 < frac <= 1')
    m = max(1, int(frac * n_cols))
    return int(np.random.default_rng(seed).integers(0, n_cols - m + 1)), m


def signguard_sample(n, n_samples=50, seed=0):
    """The rows SignGuard estimates its bandwidth from, drawn on the host: min(n, n_samples) distinct row numbers as int32,
    np.random.default_rng(seed).choice(n, size, replace=False), or arange(n) when n_samples >= n."""
    n, n_samples = int(n), int(n_samples)
    if n < 1 or n_samples < 1:
        raise ValueError('signguard_sample: n and n_samples must be >= 1')
    if n_samples >= n:
        return np.arange(n, dtype=np.int32)
    return np.random.default_rng(seed).choice(n, size=n_samples, replace=False).astype(np.int32)


def bucketing_permutation(n, seed=0):
    """Bucketing's shuffle of the n clients, drawn on the host so that the library stays deterministic:
    np.random.default_rng(seed).permutation(n) as int32."""
    n = int(n)
    if n < 1:
        raise ValueError('bucketing_permutation: n must be >= 1')
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


class _DeviceF64:
    """A span of device doubles for torch.as_tensor (the all-reduce callback's buffer belongs to the library)."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {'shape': (int(count),), 'typestr': '<f8', 'data': (int(ptr), False), 'version': 2}


class EngineError(RuntimeError):
    pass


def _check(rc):
    if rc == _native.OK:
        return
    msg = _native.last_error()
    if rc == _native.E_PRECONDITION:
        raise AssertionError(msg)            # the reference asserts (defences.py:25, 56)
    if rc == _native.E_NO_WINNER:
        raise KeyError(-1)                   # the reference pops key -1 from its dict (defences.py:65)
    if rc == _native.E_INVALID:
        raise ValueError(msg)
    if rc == _native.E_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise EngineError('libbyzagg error %d: %s' % (rc, msg))


def _torch():
    """The one lazy import: the engine loads and runs on a host without torch."""
    import torch
    return torch


def _is_torch(x):
    return type(x).__module__.split('.')[0] == 'torch'


def _vp(x):
    """A void* for tests and scripts that call the library themselves; the engine passes its ints as they are."""
    return ctypes.c_void_p(int(x)) if x else None


def _is_device(x):
    return isinstance(x, DeviceBuffer) or (_is_torch(x) and x.is_cuda)


def _stream_of(t):
    return _torch().cuda.current_stream(t.device).cuda_stream


def _to_host(v):
    """numpy from a torch tensor (wherever it lives) or from anything numpy takes."""
    return v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)


def _hp(a):
    """The address of a host array, None for None.  (Device addresses, streams and these are Python ints: the prototypes
    of _native.load() turn an int or None into a void*.)"""
    return None if a is None else a.ctypes.data


# byz_minmax_params' codes (include/byzagg.h: BYZ_MINMAX_KIND_*, BYZ_MINMAX_PERTURB_*)
MINMAX_KINDS = {'minmax': 0, 'minsum': 1}
MINMAX_PERTURBATIONS = {'unit': 0, 'std': 1, 'sign': 2, 'custom': 3}
# byz_foolsgold_params' normalise (include/byzagg.h: BYZ_FOOLSGOLD_NORMALISE_*)
FOOLSGOLD_NORMALISE = {'count': 0, 'sum': 1}


class DeviceBuffer:
    """Raw device memory owned through the C ABI (lets a host without torch keep data on the GPU)."""

    def __init__(self, engine, shape, dtype):
        self.engine = engine
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        ptr = ctypes.c_void_p()
        _check(engine.lib.byz_malloc(engine.ctx, max(self.nbytes, 4), ctypes.byref(ptr)))
        self.ptr = ptr.value

    def upload(self, array):
        array = np.ascontiguousarray(array, dtype=self.dtype)
        assert array.nbytes == self.nbytes
        _check(self.engine.lib.byz_upload(self.engine.ctx, self.ptr, _hp(array), self.nbytes, None))
        self.engine.synchronize()
        return self

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        _check(self.engine.lib.byz_download(self.engine.ctx, _hp(out), self.ptr, self.nbytes, None))
        self.engine._synced(None)
        return out

    def free(self):
        if self.ptr and self.engine.ctx:
            self.engine.lib.byz_free(self.engine.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Distances:
    """What `_krum_create_distances` returns here: the N x N fp32 distance matrix, resident on the GPU.

    The reference returns a dict of dicts (defences.py:16-21); `to_dict()` rebuilds that form, with the same
    key order (1, 0, 2, ...), for code that wants to look inside.
    """

    def __init__(self, buffer, n):
        self.buffer, self.n = buffer, n

    @property
    def ptr(self):
        return self.buffer.ptr

    def numpy(self):
        return self.buffer.numpy()

    def to_dict(self):
        from collections import defaultdict
        dense = self.numpy()
        out = defaultdict(dict)
        for i in range(self.n):
            for j in range(i):
                out[i][j] = out[j][i] = dense[i, j]
        return out


class _Operand:
    """Anything handed to a kernel: device pointer, shape, for a matrix the leading dimension, and `keep`, what holds the
    memory -- the caller's torch tensor or DeviceBuffer, or a temporary of this call (an upload, or the copy torch made to
    convert).  `torch_like` is the tensor when it is one; `stream` is then torch's current stream on its device."""

    def __init__(self, ptr, shape, keep, torch_like=None, ld=None):
        self.ptr, self.shape, self.keep, self.torch_like, self.ld = ptr, tuple(int(s) for s in shape), keep, torch_like, ld
        self.size = int(np.prod(self.shape))

    rows = property(lambda self: self.shape[0])
    cols = property(lambda self: self.shape[1])
    stream = property(lambda self: None if self.torch_like is None else _stream_of(self.torch_like))


# The refusal texts of the operand kinds (_Call.operand): %(n)d is the expected count, %(got)d the count found.
_F64 = {'buffer': 'a DeviceBuffer here must hold %(n)d float64 values',
        'device': 'the vector lives on %(device)s, this engine drives cuda:%(engine)d', 'length': 'expected %(n)d values, got %(got)d'}
_ROWS = {'buffer': 'a DeviceBuffer row_index must hold int32', 'kind': 'row_index must hold integers, got %(dtype)s',
         'range': 'row_index out of range: [%(lo)d, %(hi)d] for %(n)d rows'}


def _f32(length):
    """float32 vectors used where they are; `length` is the caller's text for a wrong length."""
    return {'layout': 'device vectors must be contiguous float32', 'length': length}


_DIFFER = _f32('vector lengths differ: %(n)d and %(got)d')


def _i32(what):
    return {'buffer': 'a DeviceBuffer of %s must hold %%(n)d int32 values' % what, 'kind': what + ' must be integers, got %(dtype)s',
            'device': 'the %s live on %%(device)s, this engine drives cuda:%%(engine)d' % what,
            'length': 'expected %%(n)d %s, got %%(got)d' % what}


def _ints(what):
    """int32 or int64 arrays used where they are (Auror's votes, bad flags and counts)."""
    return dict(_i32(what), buffer='a DeviceBuffer of %s must hold %%(n)d integers of the width the call states' % what,
                layout='device %s must be contiguous and of the width the call states' % what)


def _lists(what):
    return {'buffer': 'a DeviceBuffer of neighbour lists must hold int32', 'kind': 'neighbour lists must hold integers, got %(dtype)s',
            'device': 'the neighbour lists live on %(device)s, this engine drives cuda:%(engine)d',
            'shape': 'expected %%(n)d %s, got shape %%(shape)r' % what}


class _Call:
    """One engine call that launches work: it collects the operands, and from them fixes the stream (torch's current one
    when any operand is a torch tensor, else `stream`: None is the library's default), where the outputs go (beside the
    operand that leads: torch for torch, a DeviceBuffer otherwise) and the kind of the result (numpy when what leads came
    from the host).

    The lifetime rule, in one place: a device temporary this call made (`upload`, `temporary`) must outlive the kernels that
    read it, so on exit this call's stream is synchronised if there is such a temporary and work was launched on the stream
    (`run`) with nothing synchronising it since -- synchronize(), check(), an *_info read and a library call that fills a
    host out-parameter do, and a download does for the default stream.  The caller's own tensors and DeviceBuffers never
    cause a synchronisation, nor do the copies torch makes: its allocator orders their reuse on the stream of the launch."""

    def __init__(self, engine, stream=None):
        self.engine, self.stream, self.like, self.resident, self.temps, self._torch_stream = engine, stream, None, False, [], False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and self.temps:
            self.settle()

    def settle(self):
        if self.engine._in_flight(self.stream):
            self.engine.synchronize(self.stream)

    @property
    def host(self):
        return self.like is None and not self.resident

    def temporary(self, buf):
        self.temps.append(buf)
        return buf

    def upload(self, array):
        return self.temporary(self.engine.to_device(array))

    def beside(self, tensor, on_its_stream=True):
        """The outputs go beside `tensor`, a torch CUDA tensor that is no operand (on_its_stream: and the work to its stream)."""
        self.like = tensor
        if on_its_stream:
            self.stream, self._torch_stream = _stream_of(tensor), True

    def _adopt(self, op, leads):
        if op.torch_like is not None:
            if not self._torch_stream:          # (every torch operand is on this engine's GPU: one lookup serves them all)
                self.stream, self._torch_stream = op.stream, True
            if leads:
                self.like = op.torch_like
        elif leads and not any(op.keep is t for t in self.temps):
            self.resident = True
        return op

    def matrix(self, g, needs=None):
        """The gradient matrix (or its _Operand): used where it is when device-resident; a host matrix is staged, or refused
        under the name `needs` of a method that takes device-resident matrices only."""
        m = g if isinstance(g, _Operand) else self.engine._device_matrix(g)
        if m is None:
            if needs:
                raise ValueError('%s() takes a device-resident matrix' % needs)
            m = self.engine._device_matrix(self.upload(self.engine._host_matrix(g)))
        return self._adopt(m, True)

    def distances(self, distances):
        """_as_distances, with the dense matrix it may have uploaded as this call's temporary."""
        d, keys = self.engine._as_distances(distances)
        if d is not distances:
            self.temporary(d)
        return d, keys

    def as_it_lies(self, v, leads=False):
        """A device-resident operand on the caller's word: the address of a torch tensor or a DeviceBuffer, nothing checked."""
        op = _Operand(v.data_ptr(), v.shape, v, torch_like=v) if _is_torch(v) else _Operand(v.ptr, v.shape, v)
        return self._adopt(op, leads)

    def operand(self, v, dtype, says, shape=None, convert=True, rows=None, leads=False):
        """A vector, index list or second matrix of `dtype` -> _Operand.  A DeviceBuffer or a torch CUDA tensor is used where
        it is, anything else (numpy, a torch CPU tensor, a list) is uploaded.
        says: the refusal texts of this kind of operand (_F64, _ROWS, _f32(), _i32(), _lists()); it is what keeps every
        caller's wording.  A kind without a 'buffer' text asserts a DeviceBuffer's dtype, as it always has.
        shape: an int is the expected number of entries (the operand is flattened), a tuple the expected shape (None: any
        extent), None is any flat length.
        convert: a torch CUDA tensor of another dtype or layout is converted (it must be on this engine's GPU), else refused.
        rows: every entry must lie in [0, rows) -- for a torch tensor one reduction and a host synchronisation, a
        DeviceBuffer is the caller's word.  leads: the outputs go beside this operand (see _Call)."""
        dtype, flat = np.dtype(dtype), not isinstance(shape, tuple)
        fields = {'n': shape if flat else shape[0], 'engine': self.engine.device}
        if isinstance(v, DeviceBuffer):
            size = int(np.prod(v.shape))
            fields['n'] = size if fields['n'] is None else fields['n']
            if 'buffer' not in says:
                assert v.dtype == dtype
            elif v.dtype != dtype or ('%(n)d' in says['buffer'] and shape is not None and size != shape):   # (one text for both)
                raise ValueError(says['buffer'] % fields)
            op = _Operand(v.ptr, (size,) if flat else v.shape, v)
        elif _is_torch(v) and v.is_cuda:
            torch = _torch()
            want = getattr(torch, dtype.name)
            if convert:
                if v.device.index != self.engine.device:
                    raise ValueError(says['device'] % dict(fields, device=v.device))
                v = v.to(want).contiguous()
            elif v.dtype != want or not v.is_contiguous():
                raise ValueError(says['layout'])
            if flat:
                v = v.reshape(-1)
            if rows is not None and v.numel():
                self._in_range(says, int(v.min().item()), int(v.max().item()), rows)
            op = _Operand(v.data_ptr(), v.shape, v, torch_like=v)
        else:
            host = _to_host(v)
            if dtype.kind == 'i' and host.dtype.kind not in 'iu':
                raise ValueError(says['kind'] % {'dtype': host.dtype})
            host = host.reshape(-1) if flat else host
            if rows is not None and host.size:
                self._in_range(says, host.min(), host.max(), rows)        # (before the cast: it could wrap a wide index)
            buf = self.upload(np.ascontiguousarray(host, dtype=dtype))
            op = _Operand(buf.ptr, buf.shape, buf)
        if flat and shape is not None and op.size != shape:
            raise ValueError(says['length'] % dict(fields, got=op.size))
        if not flat and (len(op.shape) != len(shape) or any(s is not None and s != n for s, n in zip(shape, op.shape))):
            raise ValueError(says['shape'] % dict(fields, shape=op.shape))
        return self._adopt(op, leads)

    @staticmethod
    def _in_range(says, lo, hi, rows):
        if lo < 0 or hi >= rows:
            raise ValueError(says['range'] % {'lo': lo, 'hi': hi, 'n': rows})

    def written(self, v, n, what):
        """A float32 vector of n entries the call writes: it must already be on the device."""
        if not _is_device(v):
            raise ValueError('%s must be a device-resident float32 vector of %d entries' % (what, n))
        return self.operand(v, np.float32, _f32(what + ' has %(got)d entries, expected %(n)d'), n, convert=False)

    def out(self, shape, dtype=np.float32, want=True):
        """An output array (a length or a shape) -> (array, device pointer): a torch tensor beside a torch operand, a
        DeviceBuffer otherwise; (None, None) when it is not wanted -- the library takes a null pointer then."""
        if not want:
            return None, None
        shape = tuple(int(n) for n in shape) if isinstance(shape, tuple) else (int(shape),)
        if self.like is not None:
            torch = _torch()
            t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.like.device)   # float32, int32, float64
            return t, t.data_ptr()
        b = DeviceBuffer(self.engine, shape, dtype)
        return b, b.ptr

    def run(self, rc, reads_back=False):
        """The return code of the library call that launched this call's work; reads_back: it filled a host out-parameter,
        so the library waited for the kernels."""
        _check(rc)
        self.engine._launched(self.stream, waited=reads_back)

    def numpy(self, buf):
        """A DeviceBuffer of this call's results, downloaded.  The download waits for the default stream only."""
        if self.stream:
            self.settle()
        return buf.numpy()

    def result(self, x):
        """The result in the caller's kind: numpy where the inputs came from the host, else as allocated."""
        if isinstance(x, tuple):
            return tuple(self.result(v) for v in x)
        return self.numpy(x) if self.host and isinstance(x, DeviceBuffer) else x


class Engine:
    def __init__(self, device=None):
        self.lib = _native.load()
        if device is None:
            device = int(os.environ.get('BYZ_DEVICE', os.environ.get('LOCAL_RANK', '0')))
        ctx = ctypes.c_void_p()
        _check(self.lib.byz_ctx_create(int(device), ctypes.byref(ctx)))
        self.ctx = ctx
        self.device = int(device)
        self._assemble_key = None     # what the context's device-side pointer table holds (assemble_rows)
        self._unsynced, self._last = set(), 0    # streams with work launched and not synchronised since; the last launch's

    def close(self):
        if getattr(self, 'ctx', None):
            self.lib.byz_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory helpers -----------------------------------------------------------------------
    def empty(self, shape, dtype=np.float32):
        return DeviceBuffer(self, shape, dtype)

    def to_device(self, array):
        array = np.ascontiguousarray(array)
        return DeviceBuffer(self, array.shape, array.dtype).upload(array)

    def stage(self, g):
        """(matrix, was_host): `g` itself when it is device-resident, else a DeviceBuffer holding the host matrix -- for a
        caller that runs several calls on one upload and brings the last result back itself."""
        if self._device_matrix(g) is not None:
            return g, False
        return self.to_device(self._host_matrix(g)), True

    def reserve(self, n_rows, n_cols):
        _check(self.lib.byz_ctx_reserve(self.ctx, int(n_rows), int(n_cols)))

    def synchronize(self, stream=None):
        _check(self.lib.byz_stream_sync(self.ctx, stream))
        self._synced(stream)

    def check(self, stream=None):
        """Synchronise and raise if a kernel of an asynchronous call flagged a failure on the device."""
        _check(self.lib.byz_ctx_check(self.ctx, stream))
        self._synced(stream)

    def _launched(self, stream, waited=False):
        self._last = int(stream or 0)
        (self._unsynced.discard if waited else self._unsynced.add)(self._last)

    def _synced(self, stream):
        self._unsynced.discard(int(stream or 0))

    def _in_flight(self, stream):
        return int(stream or 0) in self._unsynced

    def _read(self, fn, types, *tail):
        """The host out-parameters of an *_info or counter function, as Python values (the library synchronises)."""
        outs = [t() for t in types]
        _check(fn(self.ctx, *[ctypes.byref(o) for o in outs], *tail))
        self._unsynced.discard(self._last)      # (the library synchronises the stream of the rule's last call)
        return [o.value for o in outs]

    def _device_matrix(self, g):
        """torch CUDA tensor / DeviceBuffer -> _Operand; None for host arrays."""
        if isinstance(g, DeviceBuffer):
            assert g.dtype == np.float32 and len(g.shape) == 2
            return _Operand(g.ptr, g.shape, g, ld=g.shape[1])
        if _is_torch(g):
            if not g.is_cuda:
                return None
            if g.dtype != _torch().float32 or g.dim() != 2 or g.stride(1) != 1:
                raise ValueError('device matrices must be 2-D float32 with unit column stride')
            if g.device.index != self.device:
                raise ValueError('the matrix lives on %s, this engine drives cuda:%d' % (g.device, self.device))
            return _Operand(g.data_ptr(), g.shape, g, torch_like=g, ld=g.stride(0))
        return None

    @staticmethod
    def _host_matrix(g):
        g = _to_host(g)
        if g.ndim != 2:
            raise ValueError('expected a 2-D gradient matrix, got shape %r' % (g.shape,))
        return np.ascontiguousarray(g, dtype=np.float32)

    def _allreduce_callback(self, all_reduce):
        """all_reduce(tensor) as the library's byz_allreduce_f64_fn; the caller holds the returned object until the library
        call has returned."""
        device = self.device

        def reduce_on_ranks(user, buf, count, stream):
            try:
                if all_reduce is not None:
                    all_reduce(_torch().as_tensor(_DeviceF64(buf, count), device='cuda:%d' % device))
                return 0
            except Exception:      # noqa: BLE001  (a Python exception must not unwind through the C frames)
                return 1
        return _native.ALLREDUCE_F64_FN(reduce_on_ranks)

    # ---- defences.py -------------------------------------------------------------------------
    def defend_host(self, name, g, users_count, corrupted_count, check_assert=True, want_aux=False):
        """One call for a host matrix: upload, aggregate, download (the numpy drop-in path)."""
        g = self._host_matrix(g)
        n, d = g.shape
        out = np.empty(d, dtype=np.float32)
        theta = max(int(users_count) - 2 * int(corrupted_count), 1)
        aux = np.full(max(theta, 1), -1, dtype=np.int32) if want_aux else None
        _check(self.lib.byz_defend_host(self.ctx, NAME_TO_ID[name], _hp(g), n, d, int(users_count), int(corrupted_count),
                                        int(bool(check_assert)), _hp(out), _hp(aux)))
        return (out, aux) if want_aux else out

    def no_defense(self, g, users_count=None, corrupted_count=None):
        dm = self._device_matrix(g)
        if dm is None:
            return self.defend_host('NoDefense', g, 0, 0)
        with _Call(self) as c:
            m = c.matrix(dm)
            out, ptr = c.out(m.cols)
            c.run(self.lib.byz_no_defense_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, ptr, c.stream))
        return out

    def pairwise_distances(self, g):
        with _Call(self) as c:
            m = c.matrix(g)
            dist = DeviceBuffer(self, (m.rows, m.rows), np.float32)
            c.run(self.lib.byz_pairwise_distances_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, dist.ptr, c.stream))
            self.check(c.stream)
        return Distances(dist, m.rows)

    def gram(self, g):
        """fp64 Gram matrix of a device-resident slice (the D-sharded multi-GPU path all-reduces these)."""
        with _Call(self) as c:
            m = c.matrix(g, needs='gram')
            out, ptr = c.out((m.rows, m.rows), np.float64)
            c.run(self.lib.byz_gram_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, ptr, c.stream))
        return out

    def _row_index(self, c, row_index, m, validate):
        """row_index (None: every row) -> (device pointer, count).  The kernel reads int32 indices straight from device
        memory: anything else is converted, and (unless the caller vouches for a torch tensor) checked against the matrix
        height, because an out-of-range index is an out-of-bounds read on the GPU.  A torch tensor must be on the matrix's GPU."""
        if row_index is None:
            return None, m.rows
        if _is_torch(row_index):
            if not row_index.is_cuda or (m.torch_like is not None and row_index.device != m.torch_like.device) \
                    or row_index.device.index != self.device:
                raise ValueError('row_index must live on the GPU of the matrix (cuda:%d), got %s'
                                 % (self.device, row_index.device))
            torch = _torch()
            if row_index.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
                raise ValueError('row_index must hold integers, got %s' % row_index.dtype)
        idx = c.operand(row_index, np.int32, _ROWS, rows=m.rows if validate or not _is_torch(row_index) else None)
        return idx.ptr, idx.size

    def gram_share_add(self, panel, row_index, share_count, share_index, gram):
        """`gram` (the caller's N x N fp64 device buffer, zeroed before the first panel) += this rank's share of the Gram
        tiles of `panel`: the per-panel N x N addition pass of the clients layout folded into the reduction kernel."""
        with _Call(self) as c:
            m = c.matrix(panel, needs='gram_share_add')
            idx_ptr, n_rows = self._row_index(c, row_index, m, validate=False)
            if tuple(gram.shape) != (n_rows, n_rows):
                raise ValueError('the accumulator must be %d x %d' % (n_rows, n_rows))
            # the kernel read-modify-writes N * N doubles at this address: anything else than a contiguous fp64 buffer on the
            # panel's device would corrupt memory silently
            if _is_torch(gram):
                if gram.dtype != _torch().float64 or not gram.is_contiguous() or not gram.is_cuda:
                    raise ValueError('the accumulator must be a contiguous float64 CUDA tensor')
                if m.torch_like is not None and gram.device != m.torch_like.device:
                    raise ValueError('the accumulator lives on %s, the panel on %s' % (gram.device, m.torch_like.device))
            elif not isinstance(gram, DeviceBuffer):
                raise ValueError('the accumulator must be a torch CUDA tensor or a DeviceBuffer')
            elif gram.dtype != np.float64:
                raise ValueError('the accumulator must be float64')
            acc = c.as_it_lies(gram)
            c.run(self.lib.byz_gram_share_add_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, int(share_count),
                                                  int(share_index), acc.ptr, c.stream))
        return gram

    def gram_share(self, panel, row_index, share_count, share_index):
        """This rank's share of the Gram tiles of `panel` (a device matrix every rank holds, e.g. an all-gathered column
        panel): zeros outside the share, so the ranks' outputs SUM to the Gram.  `row_index` (int32, on the device, or
        None): logical row r is panel[row_index[r]] -- skips the padding rows of an unevenly sharded gather."""
        with _Call(self) as c:
            m = c.matrix(panel, needs='gram_share')
            idx_ptr, n_rows = self._row_index(c, row_index, m, validate=False)
            out, ptr = c.out((n_rows, n_rows), np.float64)
            c.run(self.lib.byz_gram_share_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, int(share_count),
                                              int(share_index), ptr, c.stream))
        return out

    def near_pairs_count(self, stream=None):
        """Pairs the last distance kernel could not resolve through the Gram identity (synchronises)."""
        return self._read(self.lib.byz_near_pairs_count, [ctypes.c_int64], stream)[0]

    def near_pairs_sqdist(self, g, count, row_index=None):
        """Per listed pair, the sum over g's columns of the squared fp32 difference (fp64): this rank's part."""
        with _Call(self) as c:
            m = c.matrix(g, needs='near_pairs_sqdist')
            idx_ptr, _ = self._row_index(c, row_index, m, validate=False)
            sq, sq_ptr = c.out(count, np.float64)
            c.run(self.lib.byz_near_pairs_sqdist_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, idx_ptr, sq_ptr, c.stream))
        return sq

    def near_pairs_apply(self, sq, distances, stream=None):
        """distances[i, j] = sqrt(sq[p]) for every listed pair, then identical rows are made to tie exactly again."""
        with _Call(self, stream) as c:
            sq = c.as_it_lies(sq)
            c.run(self.lib.byz_near_pairs_apply_dev(self.ctx, sq.ptr, int(distances.n), distances.ptr, c.stream))
            self.check(c.stream)

    def distances_from_gram(self, gram, n, stream=None, local_columns=None, all_reduce=None):
        """Distances from an (all-reduced) fp64 Gram.  The Gram identity cannot resolve nearly coincident rows, so the
        kernel lists those pairs; with `local_columns` (this rank's column slice of G) they are re-evaluated on the
        difference itself: per-rank sums of squared differences, `all_reduce(tensor)` over the ranks when given, then
        applied -- the same result as the single-GPU path, which does all of it inside byz_pairwise_distances_dev.
        Without `local_columns` the list is left for the caller (near_pairs_count / _sqdist / _apply)."""
        with _Call(self, stream) as c:
            gram = c.as_it_lies(gram)
            dist = Distances(DeviceBuffer(self, (n, n), np.float32), n)
            c.run(self.lib.byz_distances_from_gram_dev(self.ctx, gram.ptr, int(n), dist.ptr, c.stream))
            if local_columns is None:
                self.check(c.stream)
                return dist
            count = self.near_pairs_count(c.stream)
            if count:
                sq = self.near_pairs_sqdist(local_columns, count)
                if all_reduce is not None:
                    all_reduce(sq)
                self.near_pairs_apply(sq, dist, c.stream)
        return dist

    def _as_distances(self, distances):
        """-> (Distances, keys): `keys[c]` is the reference's row index of row c of the dense matrix, or None when
        they coincide.

        A dict is what the reference's own loops pass around (defences.py:16-21, and :61-68 where Bulyan pops the
        winner's row and column before the next `krum(..., distances, True)`): any subset of rows may be present,
        in dict order.  The kernels visit rows in the order 1, 0, 2, 3, ..., which IS the dict order of a complete
        dict; for a dict with rows removed the dense matrix lists the keys in dict order with the first two
        swapped, so that the same kernel order walks them as the reference's `for user in distances.keys()` does."""
        if isinstance(distances, Distances):
            return distances, None
        if isinstance(distances, dict):
            keys = list(distances.keys())
            m = len(keys)
            if m >= 2:
                keys[0], keys[1] = keys[1], keys[0]
            position = {k: c for c, k in enumerate(keys)}
            dense = np.full((m, m), np.inf, dtype=np.float32)
            for k, row in distances.items():
                if len(row) != m - 1:
                    raise ValueError('distance dict is not square: row %r has %d entries, %d rows present'
                                     % (k, len(row), m))
                c = position[k]
                for j, v in row.items():
                    dense[c, position[j]] = v
            plain = keys == list(range(m))
            return Distances(self.to_device(dense), m), (None if plain else keys)
        dense = np.ascontiguousarray(distances, dtype=np.float32)
        if dense.ndim != 2 or dense.shape[0] != dense.shape[1]:
            raise ValueError('distances must be a square matrix')
        return Distances(self.to_device(dense), dense.shape[0]), None

    def krum_select(self, distances, users_count, corrupted_count):
        """The selection loop of defences.py:27-37 on a distance matrix; returns the index (or -1)."""
        with _Call(self) as c:
            d, keys = c.distances(distances)
            idx = ctypes.c_int32(-2)
            c.run(self.lib.byz_krum_select_dev(self.ctx, d.ptr, d.n, int(users_count), int(corrupted_count),
                                               ctypes.byref(idx), None, None), reads_back=True)
        idx = int(idx.value)
        return idx if (keys is None or idx < 0) else keys[idx]

    def krum(self, g, users_count, corrupted_count, distances=None, return_index=False, debug=False, *, check=True):
        """defences.krum (defences.py:23-42).  Device-resident `g` without `return_index`: the winning row is copied on
        the device and nothing needs to cross to the host, but a kernel can only FLAG a failure there (a Gram chunk that
        never got its ticket, helpers that lost their worker: the sticky status word) -- so by default the call ends with
        `self.check(stream)` (one synchronisation) and raises instead of returning a row picked from invalid distances.
        `check=False` (keyword only: the positional slot behind `return_index` is the reference's `debug`, accepted and
        ignored) keeps the call asynchronous; the caller then owes an `engine.check()` before it uses the result."""
        if not return_index:
            # defences.py:24-25 (the message says +3, the check is +1)
            assert users_count >= 2 * corrupted_count + 1, (
                'users_count>=2*corrupted_count + 3', users_count, corrupted_count)
        if distances is not None:
            idx = self.krum_select(distances, users_count, corrupted_count)
            if return_index:
                return idx
            return self._row(g, idx)
        dm = self._device_matrix(g)
        if dm is None:
            out, aux = self.defend_host('Krum', g, users_count, corrupted_count, check_assert=False, want_aux=True)
            if return_index:
                return int(aux[0])
            if isinstance(g, np.ndarray) and g.ndim == 2:
                # the reference returns users_grads[index] -- a VIEW of the caller's matrix (defences.py:42), -1 = numpy's last
                # row when no score beat 1e20 -- and since round 6 so does the host path (missing 6)
                return g[int(aux[0])]
            return out
        with _Call(self) as c:
            m = c.matrix(dm)
            idx = ctypes.c_int32(-2)
            out, ptr = c.out(m.cols, want=not return_index)
            # the winning row is copied on the device; the index crosses to the host (one sync) only when asked for
            c.run(self.lib.byz_krum_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(users_count), int(corrupted_count), 0, ptr,
                                        ctypes.byref(idx) if return_index else None, c.stream), reads_back=return_index)
            if return_index:
                return int(idx.value)      # (the library read the status word together with the index)
            if check:
                self.check(c.stream)
        return out

    def _row(self, g, idx):
        """Row `idx` of the caller's matrix, in the caller's own container type (negative idx as numpy)."""
        if isinstance(g, DeviceBuffer):
            return g.numpy()[idx]
        return g[idx]

    def trimmed_mean(self, g, users_count=None, corrupted_count=0, row_index=None, validate_index=True):
        dm = self._device_matrix(g)
        if dm is None:
            if row_index is not None:
                g = self._host_matrix(g)[np.asarray(row_index)]
            return self.defend_host('TrimmedMean', g, 0, corrupted_count)
        with _Call(self) as c:
            m = c.matrix(dm)
            idx_ptr, n_rows = self._row_index(c, row_index, m, validate_index)
            if n_rows == 0:
                raise ValueError('row_index selects no rows')
            out, ptr = c.out(m.cols)
            c.run(self.lib.byz_trimmed_mean_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, int(corrupted_count), ptr,
                                                c.stream))
        return out

    def _rank_rule(self, g, trim_count, row_index, validate_index):
        """The two coordinate-wise rank rules share their plumbing: trim_count None is the median."""
        dm = self._device_matrix(g)
        if dm is None:
            g = self._host_matrix(g)
            if row_index is not None:
                g = np.ascontiguousarray(g[np.asarray(row_index)])
            n, d = g.shape
            if n == 0:
                raise ValueError('row_index selects no rows')
            out = np.empty(d, dtype=np.float32)
            if trim_count is None:
                _check(self.lib.byz_coordinate_median_host(self.ctx, _hp(g), n, d, _hp(out)))
            else:
                _check(self.lib.byz_rank_trimmed_mean_host(self.ctx, _hp(g), n, d, int(trim_count), _hp(out)))
            return out
        with _Call(self) as c:
            m = c.matrix(dm)
            idx_ptr, n_rows = self._row_index(c, row_index, m, validate_index)
            if n_rows == 0:
                raise ValueError('row_index selects no rows')
            out, ptr = c.out(m.cols)
            if trim_count is None:
                c.run(self.lib.byz_coordinate_median_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, ptr, c.stream))
            else:
                c.run(self.lib.byz_rank_trimmed_mean_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, int(trim_count), ptr,
                                                         c.stream))
        return out

    def coordinate_median(self, g, row_index=None, validate_index=True):
        """Per column np.median of the float32 rows (of g[row_index] when given), bit for bit; a NaN anywhere in a column
        makes it NaN.  Device tensors, strided views and host matrices as `trimmed_mean` takes them."""
        return self._rank_rule(g, None, row_index, validate_index)

    def rank_trimmed_mean(self, g, trim_count, row_index=None, validate_index=True):
        """Per column the mean of np.sort(col)[b : n - b], b = trim_count (0 <= b, 2 b < n), summed in fp64 and rounded to
        float32 once.  NaN sorts behind +inf (np.sort): up to b of them are trimmed away like any other large value."""
        if trim_count is None:
            raise ValueError('rank_trimmed_mean needs a trim count')
        return self._rank_rule(g, trim_count, row_index, validate_index)

    def _window_rule(self, g, centre, count, row_index, validate_index, want_radius):
        """window_mean (a centre given, count = keep) and phocas (centre None, count = trim_count) share their plumbing:
        (out, radius or None), device tensors, strided views and host matrices as `_rank_rule` takes them."""
        dm = self._device_matrix(g)
        if dm is None:
            g = self._host_matrix(g)
            if row_index is not None:
                if np.size(row_index) == 0:
                    raise ValueError('row_index selects no rows')
                g = np.ascontiguousarray(g[np.asarray(row_index)])
            n, d = g.shape
            # a host matrix's extent is known here: refused before the library is touched (the device path leaves it to the library)
            if centre is None and not 0 <= 2 * int(count) < n:
                raise ValueError('phocas: trim_count %d must satisfy 0 <= 2 b < %d rows' % (int(count), n))
            if centre is not None and not 1 <= int(count) <= n:
                raise ValueError('window_mean: keep %d outside 1..%d (the row count)' % (int(count), n))
            out = np.empty(d, dtype=np.float32)
            radius = np.empty(d, dtype=np.float32) if want_radius else None
            if centre is None:
                _check(self.lib.byz_phocas_host(self.ctx, _hp(g), n, d, int(count), _hp(out), None, _hp(radius)))
                return out, radius
            c_host = np.ascontiguousarray(centre.numpy() if isinstance(centre, DeviceBuffer) else _to_host(centre),
                                          dtype=np.float32).ravel()
            if c_host.size != d:
                raise ValueError('centre has %d entries, the matrix %d columns' % (c_host.size, d))
            _check(self.lib.byz_window_mean_host(self.ctx, _hp(g), n, d, _hp(c_host), int(count), _hp(out), _hp(radius)))
            return out, radius
        with _Call(self) as c:
            m = c.matrix(dm)
            idx_ptr, n_rows = self._row_index(c, row_index, m, validate_index)
            if n_rows == 0:
                raise ValueError('row_index selects no rows')
            if centre is not None:
                centre = c.operand(centre, np.float32, _f32('centre has %(got)d entries, the matrix %(n)d columns'), m.cols,
                                   convert=False)
            out, ptr = c.out(m.cols)
            radius, rptr = c.out(m.cols, want=want_radius)
            if centre is None:
                c.run(self.lib.byz_phocas_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, int(count), ptr, None, rptr,
                                              c.stream))
                return out, radius
            c.run(self.lib.byz_window_mean_dev(self.ctx, m.ptr, n_rows, m.cols, m.ld, idx_ptr, centre.ptr, int(count), ptr, rptr,
                                               c.stream))
        return out, radius

    def window_mean(self, g, centre, keep, row_index=None, validate_index=True, return_radius=False):
        """Per column the mean of the `keep` values nearest to centre[column] (1 <= keep <= n), summed in fp64 and rounded to
        float32 once: the rows are ranked by |fl32(x - c)|, ties in the order of the rows (of g[row_index] when given), every
        NaN difference behind +inf.  `centre`: a device tensor or an array of `cols` float32 values.  return_radius=True
        returns (out, radius): |x - c| of the last value kept, per column."""
        if keep is None or centre is None:
            raise ValueError('window_mean needs a centre and a keep count')
        out, radius = self._window_rule(g, centre, keep, row_index, validate_index, return_radius)
        return (out, radius) if return_radius else out

    def phocas(self, g, trim_count, row_index=None, validate_index=True):
        """Phocas (Xie, Koyejo and Gupta 2018): per column the mean of the n - b values nearest to the b-trimmed mean,
        b = trim_count (0 <= b, 2 b < n) -- window_mean(g, rank_trimmed_mean(g, b), n - b), bit for bit, in one call."""
        if trim_count is None:
            raise ValueError('phocas needs a trim count')
        return self._window_rule(g, None, trim_count, row_index, validate_index, False)[0]

    def trimmed_mean_redone(self, stream=None):
        """16-column tiles of the last trimmed mean that the ring selection handed to the general kernel."""
        return self._read(self.lib.byz_trimmed_mean_redone, [ctypes.c_int64], stream)[0]

    def bulyan_select(self, distances, users_count, corrupted_count, on_device=False):
        """The pick-and-remove loop of defences.py:59-68: theta indices in selection order.  `on_device=True` leaves
        them in a DeviceBuffer (int32) for `trimmed_mean(row_index=...)` -- no host round trip between the stages."""
        theta = int(users_count) - 2 * int(corrupted_count)
        with _Call(self) as c:
            d, keys = c.distances(distances)
            sel = DeviceBuffer(self, (max(theta, 1),), np.int32)
            c.run(self.lib.byz_bulyan_select_dev(self.ctx, d.ptr, d.n, int(users_count), int(corrupted_count), sel.ptr, None))
            return self._selection(sel, theta, keys, on_device)

    def _selection(self, sel, count, keys, on_device):
        """The first `count` rows a selection kernel wrote to `sel`, for the caller: under the caller's keys (_as_distances), or
        left on the device when asked for (plain keys only)."""
        if on_device and keys is None:
            sel.shape = (count,)
            sel.nbytes = count * 4
            return sel
        picked = sel.numpy()[:count]
        return picked if keys is None else np.asarray([keys[i] for i in picked], dtype=np.int32)

    def krum_bulyan_select(self, distances, users_count, corrupted_count, on_device=False):
        """(Krum index, Bulyan selection) from ONE distance matrix with one sort of its rows -- what a round that runs both
        defences on the same distances needs (BASELINE configs[4]); the same values `krum_select` and `bulyan_select` return."""
        theta = int(users_count) - 2 * int(corrupted_count)
        with _Call(self) as c:
            d, keys = c.distances(distances)
            sel = DeviceBuffer(self, (max(theta, 1),), np.int32)
            idx = ctypes.c_int32(-2)
            c.run(self.lib.byz_krum_bulyan_select_dev(self.ctx, d.ptr, d.n, int(users_count), int(corrupted_count),
                                                      ctypes.byref(idx), sel.ptr, None), reads_back=True)
            index = int(idx.value)
            index = index if (keys is None or index < 0) else keys[index]
            return index, self._selection(sel, theta, keys, on_device)

    def bulyan_rescored(self):
        """Rows the last Bulyan loop re-scored with the reference's sequential fp32 sums (0: every pick was clear)."""
        return self._read(self.lib.byz_bulyan_rescored, [ctypes.c_int64])[0]

    def bulyan(self, g, users_count, corrupted_count, return_selection=False):
        assert users_count >= 4 * corrupted_count + 3  # defences.py:56
        dm = self._device_matrix(g)
        if dm is None:
            if return_selection:
                out, aux = self.defend_host('Bulyan', g, users_count, corrupted_count, want_aux=True)
                return out, aux[:int(users_count) - 2 * int(corrupted_count)]
            return self.defend_host('Bulyan', g, users_count, corrupted_count)
        theta = int(users_count) - 2 * int(corrupted_count)
        with _Call(self) as c:
            m = c.matrix(dm)
            out, ptr = c.out(m.cols)
            sel, sel_ptr = c.out(max(theta, 1), np.int32, want=return_selection)
            c.run(self.lib.byz_bulyan_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(users_count), int(corrupted_count), ptr,
                                          sel_ptr, c.stream))
        return (out, sel) if return_selection else out

    # ---- Multi-Krum (Blanchard et al. 2017, section 4; not in the reference) -------------------
    @staticmethod
    def _multi_krum_m(users_count, corrupted_count, m):
        """Blanchard's default: the users_count - corrupted_count best-scored rows."""
        return int(users_count) - int(corrupted_count) if m is None else int(m)

    def multi_krum_select(self, distances, users_count, corrupted_count, m=None, on_device=False):
        """The m best Krum-scored rows of a distance matrix (a `Distances` handle, the reference's dict, or a dense matrix),
        in ranking order: ascending score (defences.py:33-34's, as `krum` forms it), a tie broken by the visit order 1, 0, 2,
        ..., every NaN last.  `on_device=True` leaves them in a DeviceBuffer (int32)."""
        m = self._multi_krum_m(users_count, corrupted_count, m)
        with _Call(self) as c:
            d, keys = c.distances(distances)
            sel = DeviceBuffer(self, (max(m, 1),), np.int32)
            c.run(self.lib.byz_multi_krum_select_dev(self.ctx, d.ptr, d.n, int(users_count), int(corrupted_count), m, sel.ptr,
                                                     None))
            return self._selection(sel, m, keys, on_device)

    def mean_rows(self, g, row_index, validate_index=True):
        """Column mean of the rows `row_index` names, in that order, with no_defense's arithmetic (sequential fp32 from
        +0.0, then / count).  `g` is device-resident; indices are checked against its height unless the caller vouches."""
        with _Call(self) as c:
            m = c.matrix(g, needs='mean_rows')
            idx_ptr, count = self._row_index(c, row_index, m, validate_index)
            if count == 0:
                raise ValueError('row_index selects no rows')
            out, ptr = c.out(m.cols)
            c.run(self.lib.byz_mean_rows_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, idx_ptr, count, ptr, c.stream))
        return out

    def multi_krum(self, g, users_count, corrupted_count, m=None, distances=None, return_selection=False):
        """Multi-Krum: np.mean(g[np.sort(selection)], axis=0) over the m (default users_count - corrupted_count) best
        Krum-scored rows; m = 1 is Krum's row, m = n_rows is no_defense.  The selection (ranking order) comes back as
        numpy for a host matrix, on the device (int32) for a device-resident one."""
        assert users_count >= 2 * corrupted_count + 1, (
            'users_count>=2*corrupted_count + 3', users_count, corrupted_count)
        mm = self._multi_krum_m(users_count, corrupted_count, m)
        dm = self._device_matrix(g)
        if distances is not None:
            selection = self.multi_krum_select(distances, users_count, corrupted_count, mm)
            rows = np.sort(selection)
            if dm is None:
                out = self.mean_rows(self.to_device(self._host_matrix(g)), rows).numpy()
            else:
                out = self.mean_rows(g, rows)
                if dm.torch_like is not None:
                    selection = _torch().from_numpy(selection).to(dm.torch_like.device)
            return (out, selection) if return_selection else out
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            out = np.empty(d, dtype=np.float32)
            sel = np.full(max(mm, 1), -1, dtype=np.int32)
            _check(self.lib.byz_multi_krum_host(self.ctx, _hp(h), n, d, int(users_count), int(corrupted_count), mm, _hp(out),
                                                _hp(sel)))
            return (out, sel[:mm]) if return_selection else out
        with _Call(self) as c:
            dm = c.matrix(dm)
            out, ptr = c.out(dm.cols)
            sel, sel_ptr = c.out(max(mm, 1), np.int32, want=return_selection)
            c.run(self.lib.byz_multi_krum_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, int(users_count), int(corrupted_count),
                                              mm, 0, ptr, sel_ptr, c.stream))
            self.check(c.stream)      # (a kernel of the distances can only flag a failure: the sticky status word)
        return (out, sel) if return_selection else out

    # ---- geometric median (smoothed Weiszfeld; RFA, Pillutla et al.; not in the reference) ----
    def row_sqdist(self, g, z):
        """sq[i] = sum_c ((double)g[i, c] - (double)z[c])^2 in fp64 (fixed order; on the difference, not through the
        Gram identity).  fp64 out: a torch tensor for a torch input, numpy for a host input, a DeviceBuffer otherwise."""
        with _Call(self) as c:
            m = c.matrix(g)
            z = c.operand(z, np.float32, _f32('z has %(got)d entries, the matrix %(n)d columns'), m.cols, convert=False)
            out, optr = c.out(m.rows, np.float64)
            c.run(self.lib.byz_row_sqdist_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, z.ptr, optr, c.stream))
            return c.result(out)

    def weighted_mean(self, g, weights, validate=True):
        """out[c] = fl32(S_c / W): S_c the sequential fp64 sum, in row order, of w_i * g[i, c] over the rows with w_i != 0,
        W = sum w_i.  The weights must be finite and >= 0; all zero gives NaN.  validate=True checks them here: for
        device-resident weights that is one reduction and a host synchronisation.  validate=False is for a caller that
        vouches for them (the kernel would carry a NaN or a negative weight into the mean)."""
        with _Call(self) as c:
            m = c.matrix(g)
            w = c.operand(weights, np.float64, _F64, m.rows)
            if validate:
                if w.torch_like is not None:
                    torch = _torch()
                    bad = bool((~torch.isfinite(w.torch_like) | (w.torch_like < 0)).any().item())
                else:
                    w_host = np.asarray(weights.numpy() if isinstance(weights, DeviceBuffer) else _to_host(weights), dtype=np.float64)
                    bad = bool((~np.isfinite(w_host) | (w_host < 0)).any())
                if bad:
                    raise ValueError('weights must be finite and >= 0')
            out, optr = c.out(m.cols)
            c.run(self.lib.byz_weighted_mean_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, w.ptr, optr, c.stream))
            return c.result(out)

    @staticmethod
    def _geomed_params(nu, max_iter, ftol):
        return _native.GeomedParams(float(nu), int(max_iter), float(ftol))

    def geometric_median_info(self):
        """(iterations, excluded_rows, objective) of the last geometric median on this engine (synchronises)."""
        return tuple(self._read(self.lib.byz_geometric_median_info, [ctypes.c_int64, ctypes.c_int64, ctypes.c_double]))

    def geometric_median(self, g, nu=1e-6, max_iter=10, ftol=1e-6, return_info=False):
        """The geometric median of the rows by smoothed Weiszfeld iterations (RFA), started at no_defense's mean; rows with
        a non-finite entry are left out when the mean is not finite.  nu = 1e-6, max_iter = 10 and ftol = 1e-6 are this
        package's defaults, not the paper's.  return_info=True also returns {iterations, objective, excluded_rows, weights}
        (weights: fp64, one per row, summing to 1 over the rows of the last update)."""
        params = self._geomed_params(nu, max_iter, ftol)
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            out = np.empty(d, dtype=np.float32)
            weights = np.empty(n, dtype=np.float64) if return_info else None
            _check(self.lib.byz_geometric_median_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(out), _hp(weights)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                out, ptr = c.out(dm.cols)
                weights, wptr = c.out(dm.rows, np.float64, want=return_info)
                c.run(self.lib.byz_geometric_median_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params), ptr,
                                                        wptr, c.stream))
        if not return_info:
            return out
        iterations, excluded, objective = self.geometric_median_info()
        return out, {'iterations': iterations, 'objective': objective, 'excluded_rows': excluded, 'weights': weights}

    # ---- centered clipping (Karimireddy, He and Jaggi 2021, Algorithm 2; not in the reference) ----
    def clip_update(self, g, v, scales):
        """out[c] = fl32(v[c] + S_c / n): S_c the sequential fp64 sum, in row order, of scales[i] * (g[i, c] - v[c]) over the
        rows with scales[i] != 0 (a row of scale 0 is not read).  One iteration of centered clipping is row_sqdist, the
        scales min(1, tau / d), then this.  The caller vouches that the scales are finite."""
        with _Call(self) as c:
            m = c.matrix(g)
            v = c.operand(v, np.float32, _f32('v has %(got)d entries, the matrix %(n)d columns'), m.cols, convert=False)
            s = c.operand(scales, np.float64, _F64, m.rows)
            out, optr = c.out(m.cols)
            c.run(self.lib.byz_clip_update_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, v.ptr, s.ptr, optr, c.stream))
            return c.result(out)

    def centered_clip_info(self):
        """(clipped_rows, excluded_rows) of the last iteration of the last centered clipping on this engine (synchronises)."""
        return tuple(self._read(self.lib.byz_centered_clip_info, [ctypes.c_int64, ctypes.c_int64]))

    def centered_clip(self, g, tau=10.0, iters=3, start=None, return_info=False):
        """Centered clipping: from v = start (None: the zero vector; the previous round's aggregate is the paper's choice),
        `iters` times v <- v + mean_i((x_i - v) * min(1, tau / |x_i - v|)).  A row at a non-finite distance is excluded: it
        adds nothing and still counts in the mean's divisor.  start=None with iters=1 is the norm-clipped mean.  tau = 10.0
        and iters = 3 are this package's choices: the literature agrees on no defaults.  return_info=True also returns
        {clipped_rows, excluded_rows, scales} of the last iteration (scales: fp64, one per row)."""
        params = _native.CclipParams(float(tau), int(iters))
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            out = np.empty(d, dtype=np.float32)
            scales = np.empty(n, dtype=np.float64) if return_info else None
            s_host = None
            if start is not None:
                s_host = np.ascontiguousarray(_to_host(start), dtype=np.float32).ravel()
                if s_host.size != d:
                    raise ValueError('start has %d entries, the matrix %d columns' % (s_host.size, d))
            _check(self.lib.byz_centered_clip_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(s_host), _hp(out),
                                                   _hp(scales)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                sptr = None if start is None else c.operand(start, np.float32, _f32('start has %(got)d entries, the matrix %(n)d columns'), dm.cols, convert=False).ptr
                out, ptr = c.out(dm.cols)
                scales, wptr = c.out(dm.rows, np.float64, want=return_info)
                c.run(self.lib.byz_centered_clip_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params), sptr, ptr,
                                                     wptr, c.stream))
        if not return_info:
            return out
        clipped, excluded = self.centered_clip_info()
        return out, {'clipped_rows': clipped, 'excluded_rows': excluded, 'scales': scales}

    # ---- FLTrust (Cao, Fang, Liu and Gong 2021; not in the reference) ----
    def row_dots(self, g, r):
        """(dot, sq): dot[i] = sum_c (double)g[i, c] * (double)r[c] and sq[i] = sum_c (double)g[i, c]^2, both fp64 in a fixed
        order, in ONE read of g (FLTrust's first pass; on one rank of the columns layout, its part over its columns).  fp64
        out: torch tensors for a torch input, numpy for a host input, DeviceBuffers otherwise."""
        with _Call(self) as c:
            m = c.matrix(g)
            r = c.operand(r, np.float32, _f32('r has %(got)d entries, the matrix %(n)d columns'), m.cols, convert=False)
            dot, dptr = c.out(m.rows, np.float64)
            sq, sptr = c.out(m.rows, np.float64)
            c.run(self.lib.byz_row_dots_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, r.ptr, dptr, sptr, c.stream))
            return c.result((dot, sq))

    def scaled_rows_sum(self, g, weights, divisor):
        """out[c] = fl32(S_c / T) where T = divisor > 0, zeros otherwise: S_c the sequential fp64 sum, in row order, of
        weights[i] * g[i, c] over the rows with weights[i] != 0 (a row of weight 0 is not read).  FLTrust's second pass; the
        divisor is one fp64 value, on the host or the device.  The caller vouches that the weights are finite."""
        with _Call(self) as c:
            m = c.matrix(g)
            w = c.operand(weights, np.float64, _F64, m.rows)
            t = c.operand(divisor, np.float64, _F64, 1)
            out, optr = c.out(m.cols)
            c.run(self.lib.byz_scaled_rows_sum_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, w.ptr, t.ptr, optr, c.stream))
            return c.result(out)

    def fltrust_info(self):
        """(trusted_rows, excluded_rows, root_ok, trust_sum) of the last FLTrust call on this engine (synchronises)."""
        trusted, excluded, ok, total = self._read(self.lib.byz_fltrust_info,
                                                  [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_double])
        return trusted, excluded, bool(ok), total

    def fltrust(self, g, root, return_info=False):
        """FLTrust: every row's trust score is the ReLU of its cosine with `root`, the gradient the server computed on its own
        root dataset; a trusted row is rescaled to the root's norm and the result is the trust-weighted mean of the rescaled
        rows.  No row trusted, or a zero or non-finite root: the zero vector.  A row whose dot product or norm is not finite
        is excluded.  return_info=True also returns {trusted_rows, excluded_rows, root_ok, trust_sum, trust, weights} (trust
        and weights: fp64, one per row)."""
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            r_host = np.ascontiguousarray(root.numpy() if isinstance(root, DeviceBuffer) else _to_host(root), dtype=np.float32).ravel()
            if r_host.size != d:
                raise ValueError('root has %d entries, the matrix %d columns' % (r_host.size, d))
            out = np.empty(d, dtype=np.float32)
            trust = np.empty(n, dtype=np.float64) if return_info else None
            weights = np.empty(n, dtype=np.float64) if return_info else None
            _check(self.lib.byz_fltrust_host(self.ctx, _hp(h), n, d, _hp(r_host), _hp(out), _hp(trust), _hp(weights)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                root = c.operand(root, np.float32, _f32('root has %(got)d entries, the matrix %(n)d columns'), dm.cols, convert=False)
                out, ptr = c.out(dm.cols)
                trust, tptr = c.out(dm.rows, np.float64, want=return_info)
                weights, wptr = c.out(dm.rows, np.float64, want=return_info)
                c.run(self.lib.byz_fltrust_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, root.ptr, ptr, tptr, wptr, c.stream))
        if not return_info:
            return out
        trusted, excluded, ok, total = self.fltrust_info()
        return out, {'trusted_rows': trusted, 'excluded_rows': excluded, 'root_ok': ok, 'trust_sum': total, 'trust': trust,
                     'weights': weights}

    # ---- SignGuard (Xu, Huang, Song and Lan, ICDCS 2022; not in the reference) ----
    def row_signs(self, g, window_start, window_len):
        """(pos, zero, neg, q): the int64 counts of positive, zero and negative values of every row over the columns
        [window_start, window_start + window_len), and q[i] = sum_c (double)g[i, c]^2 over ALL columns (row_dots' sq, bit for
        bit), in ONE read of g.  A value is counted on its bits: +0.0 and -0.0 are zeros, denormals and infinities count by
        their sign, a NaN counts nowhere.  window_len = 0 is allowed.  torch tensors for a torch input, numpy for a host input;
        for a DeviceBuffer the counts come back as numpy and q as a DeviceBuffer."""
        with _Call(self) as c:
            m = c.matrix(g)
            counts, cptr = c.out((3, m.rows), np.int64)
            q, qptr = c.out(m.rows, np.float64)
            c.run(self.lib.byz_row_signs_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(window_start), int(window_len), cptr,
                                             qptr, c.stream))
            if isinstance(counts, DeviceBuffer):
                counts = c.numpy(counts)     # (a DeviceBuffer has no row views: the three count vectors come back on the host)
            return counts[0], counts[1], counts[2], c.result(q)

    @staticmethod
    def _signguard_params(window_start, window_len, lower, upper, bandwidth, n_sample):
        lower, upper = float(lower), float(upper)
        bandwidth = 0.0 if bandwidth is None else float(bandwidth)
        if not lower >= 0.0 or not upper > lower or not bandwidth >= 0.0 or int(window_start) < 0 or int(window_len) < 1:
            raise ValueError('signguard: lower = %r must be >= 0, upper = %r > lower, bandwidth = %r >= 0 or None, the window '
                             '(%r, %r) a start >= 0 and a length >= 1' % (lower, upper, bandwidth, window_start, window_len))
        return _native.SignGuardParams(int(window_start), int(window_len), lower, upper, bandwidth, int(n_sample))

    def _signguard_sample(self, sample, n_rows, n_samples, seed, bandwidth):
        """The sampled rows as a checked host int32 array (None when the bandwidth is given)."""
        if bandwidth is not None and float(bandwidth) > 0.0:
            return None
        if sample is None:
            sample = signguard_sample(n_rows, min(int(n_samples), _native.SIGNGUARD_MAX_SAMPLES), seed)
        sample = np.ascontiguousarray(_to_host(sample).reshape(-1))
        if sample.dtype.kind not in 'iu' or sample.size < 1 or sample.size > min(n_rows, _native.SIGNGUARD_MAX_SAMPLES) or \
                sample.min() < 0 or sample.max() >= n_rows or np.unique(sample).size != sample.size:
            raise ValueError('signguard: the sample must be 1..min(n, %d) distinct row numbers in [0, %d)'
                             % (_native.SIGNGUARD_MAX_SAMPLES, n_rows))
        return sample.astype(np.int32)

    def signguard_info(self):
        """The last SignGuard selection on this engine (synchronises): {kept_rows, norm_failed_rows, outside_rows, clusters,
        seeds, bandwidth, median_norm}."""
        names = ('kept_rows', 'norm_failed_rows', 'outside_rows', 'clusters', 'seeds', 'bandwidth', 'median_norm')
        return dict(zip(names, self._read(self.lib.byz_signguard_info, [ctypes.c_int64] * 5 + [ctypes.c_double] * 2)))

    def signguard_select(self, pos, zero, neg, q, window_len, lower=0.1, upper=3.0, bandwidth=None, sample=None, n_samples=50,
                         seed=0):
        """SignGuard's selection from row_signs' counts and squared norms (host or device vectors of n entries each):
        {keep (int32 0 / 1), weights (fp64: min(1, M / norm) for a kept row, 0 otherwise), labels (int32, -1: no cluster),
        median_norm, kept} as device-resident fp64 / int32 vectors and two device doubles `mk` = (M, K); include/byzagg.h has
        the contract.  window_len is the m the shares are divided by.  Nothing synchronises; signguard_info() does."""
        n = int(q.numel()) if _is_torch(q) else int(np.prod(q.shape)) if isinstance(q, DeviceBuffer) else int(np.asarray(q).size)
        if _is_torch(q) and q.is_cuda:
            torch = _torch()
            counts = torch.stack([torch.as_tensor(v, device=q.device).reshape(-1).to(torch.int64) for v in (pos, zero, neg)])
        else:
            counts = np.stack([(v.numpy() if isinstance(v, DeviceBuffer) else _to_host(v)).reshape(-1).astype(np.int64)
                               for v in (pos, zero, neg)])
        if tuple(counts.shape) != (3, n):
            raise ValueError('expected three count vectors of %d entries' % n)
        with _Call(self) as c:
            counts = c.operand(counts, np.int64, {}, (3, n))
            q = c.operand(q, np.float64, _F64, n, leads=True)
            sample = self._signguard_sample(sample, n, n_samples, seed, bandwidth)
            params = self._signguard_params(0, window_len, lower, upper, bandwidth, 0 if sample is None else sample.size)
            sptr = None if sample is None else c.upload(sample).ptr
            keep, kptr = c.out(n, np.int32)
            weights, wptr = c.out(n, np.float64)
            labels, lptr = c.out(n, np.int32)
            mk, mptr = c.out(2, np.float64)
            c.run(self.lib.byz_signguard_select_dev(self.ctx, counts.ptr, q.ptr, n, ctypes.byref(params), sptr, kptr, wptr, lptr,
                                                    mptr, c.stream))
        return {'keep': keep, 'weights': weights, 'labels': labels, 'mk': mk}

    def signguard(self, g, frac=0.1, lower=0.1, upper=3.0, bandwidth=None, n_samples=50, seed=0, window=None, sample=None,
                  return_info=False):
        """SignGuard: rows whose norm is outside (lower, upper) x the median norm are filtered, the rows are clustered (mean
        shift, bandwidth estimated from `n_samples` sampled rows unless given) on their shares of positive, zero and negative
        values over a window of the columns, and the mean of the largest cluster's surviving rows, each clipped to the median
        norm, is returned.  No row kept: the zero vector.  The window is `window` = (start, length) or
        signguard_window(D, frac, seed); the sampled rows are `sample` or signguard_sample(n, n_samples, seed).
        return_info=True also returns signguard_info()'s dict with keep, weights and labels (one per row) and the window."""
        dm = self._device_matrix(g)
        n, d = dm.shape if dm is not None else self._host_matrix(g).shape
        c0, m = window if window is not None else signguard_window(d, frac, seed)
        if int(c0) < 0 or int(m) < 1 or int(c0) + int(m) > d:
            raise ValueError('signguard: the window (%r, %r) is outside the %d columns' % (c0, m, d))
        sample = self._signguard_sample(sample, n, n_samples, seed, bandwidth)
        params = self._signguard_params(c0, m, lower, upper, bandwidth, 0 if sample is None else sample.size)
        if dm is None:
            h = self._host_matrix(g)
            out = np.empty(d, dtype=np.float32)
            keep = np.empty(n, dtype=np.int32) if return_info else None
            weights = np.empty(n, dtype=np.float64) if return_info else None
            labels = np.empty(n, dtype=np.int32) if return_info else None
            _check(self.lib.byz_signguard_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(sample), _hp(out), _hp(keep),
                                               _hp(weights), _hp(labels)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                sptr = None if sample is None else c.upload(sample).ptr
                out, ptr = c.out(d)
                keep, kptr = c.out(n, np.int32, want=return_info)
                weights, wptr = c.out(n, np.float64, want=return_info)
                labels, lptr = c.out(n, np.int32, want=return_info)
                c.run(self.lib.byz_signguard_dev(self.ctx, dm.ptr, n, d, dm.ld, ctypes.byref(params), sptr, ptr, kptr, wptr,
                                                 lptr, c.stream))
        if not return_info:
            return out
        info = self.signguard_info()
        info.update(keep=keep, weights=weights, labels=labels, window=(int(c0), int(m)))
        return out, info

    # ---- nearest-neighbour mixing (Allouah et al., AISTATS 2023; not in the reference) ----
    def nnm_neighbours(self, distances, k):
        """(neighbours, counts) for a distance matrix (a `Distances` handle or a dense matrix, diagonal +inf): row i of
        `neighbours` (n x k int32) is i and its k - 1 nearest rows at a finite distance, ASCENDING, then -1; counts[i] their
        number.  Order: (distance, row index), -0.0 as +0.0, every NaN behind +inf.  DeviceBuffers for a `Distances` handle
        (nothing leaves the device), numpy otherwise."""
        on_device = isinstance(distances, Distances)
        if isinstance(distances, dict):
            raise ValueError('nnm_neighbours() takes a Distances handle or a dense matrix')
        k = int(k)
        with _Call(self) as c:
            d, _ = c.distances(distances)
            nbr = DeviceBuffer(self, (d.n, max(k, 1)), np.int32)
            counts = DeviceBuffer(self, (d.n,), np.int32)
            c.run(self.lib.byz_nnm_neighbours_dev(self.ctx, d.ptr, d.n, k, nbr.ptr, counts.ptr, None))
            return (nbr, counts) if on_device else (nbr.numpy(), counts.numpy())

    def nnm_mix(self, g, neighbours, counts=None, out=None):
        """Y[i] = np.mean(g[list_i], axis=0) bit for bit (the listed rows added in ascending row order, sequential fp32 from
        +0.0, divided by the list's length); a list of one row copies that row verbatim.  `neighbours`: n x k integers, every
        list ascending with -1 behind it (nnm_neighbours' form; `counts` optional).  `g` may be a column panel of a larger
        matrix (a strided view), `out` (optional, device-resident, n x columns, may be strided too) receives the result: that
        is how a matrix too large to hold twice is mixed.  The result stays on the device when `g` was there."""
        with _Call(self) as c:
            m = c.matrix(g)
            nbr = c.operand(neighbours, np.int32, _lists('lists'), (m.rows, None))
            cptr = None if counts is None else c.operand(counts, np.int32, _lists('lengths'), (m.rows,)).ptr
            if out is None:
                y, yptr = c.out((m.rows, m.cols))
                ldy = m.cols
            else:
                om = self._device_matrix(out)
                if om is None or om.shape != m.shape:
                    raise ValueError('out must be a device-resident %d x %d float32 matrix' % (m.rows, m.cols))
                y, yptr, ldy = out, om.ptr, om.ld
            c.run(self.lib.byz_nnm_mix_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, nbr.ptr, cptr, nbr.cols, yptr, ldy, c.stream))
            return c.result(y) if out is None else y

    def nnm_info(self):
        """(solo_rows, short_rows) of the last neighbour search on this engine: the rows whose list is themselves alone
        although k > 1, and the rows whose list is shorter than k (synchronises)."""
        return tuple(self._read(self.lib.byz_nnm_info, [ctypes.c_int64, ctypes.c_int64]))

    def nnm(self, g, users_count, corrupted_count, distances=None, return_neighbours=False):
        """Nearest-neighbour mixing: every row replaced by the mean of its users_count - corrupted_count nearest rows, itself
        included (nnm_neighbours, then nnm_mix); the n x D result is what a rule such as krum, trimmed_mean or
        coordinate_median then aggregates.  A row with a non-finite value mixes with nobody and comes back verbatim.  The
        result (and the lists) stay on the device when `g` was there; numpy for a host matrix."""
        k = int(users_count) - int(corrupted_count)
        dm = self._device_matrix(g)
        if distances is not None:
            with _Call(self) as c:
                if dm is not None:
                    c.matrix(dm)
                d, _ = c.distances(distances)
                nbr, counts = (c.temporary(b) for b in self.nnm_neighbours(d, k))   # the lists are ours: they must outlive the mix
                y = self.nnm_mix(g, nbr, counts)
            if not return_neighbours:
                return y
            if dm is None:
                nbr = nbr.numpy()
            elif dm.torch_like is not None:
                nbr = _torch().from_numpy(nbr.numpy()).to(dm.torch_like.device)
            return y, nbr
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            y = np.empty((n, d), dtype=np.float32)
            nbr = np.full((n, max(k, 1)), -1, dtype=np.int32) if return_neighbours else None
            _check(self.lib.byz_nnm_host(self.ctx, _hp(h), n, d, int(users_count), int(corrupted_count), _hp(y), _hp(nbr)))
            return (y, nbr) if return_neighbours else y
        with _Call(self) as c:
            dm = c.matrix(dm)
            y, yptr = c.out(dm.shape)
            nbr, nptr = c.out((dm.rows, max(k, 1)), np.int32, want=return_neighbours)
            c.run(self.lib.byz_nnm_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, int(users_count), int(corrupted_count), yptr,
                                       dm.cols, nptr, c.stream))
            self.check(c.stream)      # (a kernel of the distances can only flag a failure: the sticky status word)
        return (y, nbr) if return_neighbours else y

    # ---- the robust learning rate (Ozdayi, Kantarcioglu and Gel, AAAI 2021; not in the reference) ----
    @staticmethod
    def _theta(theta, n_rows=None):
        if isinstance(theta, bool) or int(theta) != theta:
            raise ValueError('theta must be an integer, got %r' % (theta,))
        theta = int(theta)
        if theta < 0 or (n_rows is not None and theta > n_rows):
            raise ValueError('theta = %d outside 0..%s (the row count)' % (theta, 'n' if n_rows is None else n_rows))
        return theta

    def sign_votes(self, g):
        """votes[c] = #{r : g[r, c] > 0} - #{r : g[r, c] < 0}, int32 of length D, in one read of g: +0.0, -0.0 and NaN cast
        no vote, +-inf and denormals vote by their sign.  np.sign(votes) is signSGD's majority vote.  A torch tensor for a
        torch input, numpy for a host input, a DeviceBuffer otherwise."""
        with _Call(self) as c:
            m = c.matrix(g)
            votes, vptr = c.out(m.cols, np.int32)
            c.run(self.lib.byz_sign_votes_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, vptr, c.stream))
            return c.result(votes)

    def sign_flip(self, agg, votes, theta, out=None):
        """out[c] = agg[c] with its sign bit inverted where abs(votes[c]) < theta, agg[c] verbatim elsewhere: the robust
        learning rate applied to ANY aggregate.  out=agg (device-resident) flips in place.  numpy in -> numpy out;
        device-resident in -> device-resident out."""
        theta = self._theta(theta)
        with _Call(self) as c:
            a = c.operand(agg, np.float32, _f32(None), convert=False, leads=True)
            v = c.operand(votes, np.int32, _i32('votes'), a.size)
            if out is None:
                res, optr = c.out(a.size)
            else:
                refusal = 'out must be a device-resident float32 vector of %(n)d entries'
                if c.host or not _is_device(out):
                    raise ValueError(refusal % {'n': a.size})
                res, optr = out, c.operand(out, np.float32, _f32(refusal), a.size, convert=False).ptr
            c.run(self.lib.byz_sign_flip_dev(self.ctx, a.ptr, v.ptr, a.size, theta, optr, c.stream))
            return c.result(res)

    def robust_lr_info(self):
        """The number of columns the last sign_flip or robust_lr on this engine flipped (synchronises)."""
        return self._read(self.lib.byz_robust_lr_info, [ctypes.c_int64])[0]

    def robust_lr(self, g, theta, return_votes=False):
        """The robust learning rate around the plain mean, fused: no_defense's vector (bit for bit) with the sign bit
        inverted in every column where abs(votes) < theta, the vote counted in the same walk, so g is read once.  theta is
        an integer in [0, rows]; 0 returns no_defense's bits.  return_votes=True also returns the int32 votes."""
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            theta = self._theta(theta, n)
            out = np.empty(d, dtype=np.float32)
            votes = np.empty(d, dtype=np.int32) if return_votes else None
            _check(self.lib.byz_robust_lr_host(self.ctx, _hp(h), n, d, theta, _hp(out), _hp(votes)))
            return (out, votes) if return_votes else out
        theta = self._theta(theta, dm.rows)
        with _Call(self) as c:
            dm = c.matrix(dm)
            out, optr = c.out(dm.cols)
            votes, vptr = c.out(dm.cols, np.int32, want=return_votes)
            c.run(self.lib.byz_robust_lr_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, theta, optr, vptr, c.stream))
        return (out, votes) if return_votes else out

    # ---- s-bucketing (Karimireddy, He and Jaggi, ICLR 2022; not in the reference) ----
    def bucket_means(self, g, s, perm=None):
        """The ceil(n / s) x D matrix of bucket means: row b is np.mean(g[perm[b*s:(b+1)*s]], axis=0) bit for bit (the
        bucket's rows added in list order, sequential fp32 from +0.0, divided by the bucket's length; the last bucket may be
        short).  `perm`: a permutation of range(n) (`bucketing_permutation`), None for the identity; a host array is checked,
        a device-resident one (torch CUDA tensor, DeviceBuffer of int32) is the caller's word -- an entry out of range is
        skipped by the kernel, never read.  s = n with the identity is no_defense's vector, s = 1 is g[perm].  `g` may be a
        column panel of a larger matrix (a strided view).  The result stays on the device when `g` was there; numpy for a host
        matrix."""
        if isinstance(s, bool) or int(s) != s:
            raise ValueError('s must be an integer, got %r' % (s,))
        s = int(s)
        dm = self._device_matrix(g)
        h = self._host_matrix(g) if dm is None else None
        n, d = dm.shape if dm is not None else h.shape
        if s < 1 or s > n:
            raise ValueError('s = %d outside 1..%d (the row count)' % (s, n))
        buckets = -(-n // s)
        if perm is not None and not _is_device(perm):
            perm = np.asarray(perm.numpy() if _is_torch(perm) else perm).reshape(-1)
            if perm.dtype.kind not in 'iu' or perm.size != n or not np.array_equal(np.sort(perm), np.arange(n)):
                raise ValueError('perm must be a permutation of range(%d)' % n)
            perm = np.ascontiguousarray(perm, dtype=np.int32)
        if dm is None:
            if _is_device(perm):
                perm = np.ascontiguousarray((perm.numpy() if isinstance(perm, DeviceBuffer) else _to_host(perm)).reshape(-1),
                                            dtype=np.int32)
            y = np.empty((buckets, d), dtype=np.float32)
            _check(self.lib.byz_bucket_means_host(self.ctx, _hp(h), n, d, _hp(perm), s, _hp(y)))
            return y
        with _Call(self) as c:
            dm = c.matrix(dm)
            pptr = None if perm is None else c.operand(perm, np.int32, _i32('perm entries'), n).ptr
            y, yptr = c.out((buckets, d))
            c.run(self.lib.byz_bucket_means_dev(self.ctx, dm.ptr, n, d, dm.ld, pptr, s, yptr, d, c.stream))
        return y

    # ---- SparseFed: global top-k with error feedback (Panda et al., AISTATS 2022; not in the reference) ----
    @staticmethod
    def _topk_k(k, n=None):
        if isinstance(k, bool) or int(k) != k:
            raise ValueError('k must be an integer, got %r' % (k,))
        k = int(k)
        if k < 0 or (n is not None and k > n):
            raise ValueError('k = %d outside 0..%s (the length)' % (k, 'n' if n is None else n))
        return k

    @staticmethod
    def _host_f32(v, n=None, writable=False):
        """A flat C-contiguous float32 host vector: `v` itself where it already is one (required when the call writes it)."""
        if writable:
            if not (isinstance(v, np.ndarray) and v.dtype == np.float32 and v.flags.c_contiguous and v.flags.writeable):
                raise ValueError('a host vector that is written must be a writable C-contiguous float32 numpy array')
            host = v.reshape(-1)
        else:
            host = np.ascontiguousarray(v.numpy() if isinstance(v, DeviceBuffer) else _to_host(v), dtype=np.float32).reshape(-1)
        if n is not None and host.size != n:
            raise ValueError('expected %d values, got %d' % (n, host.size))
        return host

    def topk_info(self):
        """{selected, threshold_key, ties, ties_taken} of the last top-k on this engine (synchronises): selected == k, the
        threshold key T = the k-th largest of bits & 0x7fffffff (0xffffffff for k = 0), the columns whose key is T and how
        many of them were taken (the first in index order)."""
        names = ('selected', 'threshold_key', 'ties', 'ties_taken')
        return dict(zip(names, self._read(self.lib.byz_topk_info, [ctypes.c_int64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int64])))

    def _topk_operands(self, c, x, add, out, residual):
        """(x, add pointer, out, out pointer, residual, residual pointer) of a device-resident top-k: `out` and `residual` are
        the caller's vectors to write, or allocated beside x and add."""
        x = c.operand(x, np.float32, _f32(None), convert=False, leads=True)
        aptr = None if add is None else c.operand(add, np.float32, _DIFFER, x.size, convert=False, leads=True).ptr
        out, optr = c.out(x.size) if out is None else (out, c.written(out, x.size, 'out').ptr)
        residual, rptr = c.out(x.size) if residual is None else (residual, c.written(residual, x.size, 'residual').ptr)
        return x, aptr, out, optr, residual, rptr

    def topk_sparsify(self, x, k, add=None, out=None, residual=None, return_info=False):
        """(out, residual) of the global top-k of w = x (add=None) or fl32(x + add): the k columns first in the order (key =
        bits(w) & 0x7fffffff descending, column ascending) keep w's bits in out and are +0.0 in residual, the others the
        other way round.  Zeros of both signs tie at key 0, both infinities rank above every finite value and a NaN above
        them; nothing is sanitised.  k: an integer in [0, n].  numpy in -> numpy out; device-resident x -> device-resident
        out.  out / residual: vectors to write (device-resident for a device x); residual=x and out=add are the in-place
        round.  return_info=True also returns topk_info()."""
        if not _is_device(x):
            xh = self._host_f32(x)
            n = xh.size
            k = self._topk_k(k, n)
            ah = self._host_f32(add, n) if add is not None else None
            oh = self._host_f32(out, n, writable=True) if out is not None else np.empty(n, dtype=np.float32)
            rh = self._host_f32(residual, n, writable=True) if residual is not None else np.empty(n, dtype=np.float32)
            _check(self.lib.byz_topk_sparsify_host(self.ctx, _hp(xh), _hp(ah), n, k, _hp(oh), _hp(rh)))
            oh, rh = (out if out is not None else oh), (residual if residual is not None else rh)     # the caller's own arrays
            return (oh, rh, self.topk_info()) if return_info else (oh, rh)
        with _Call(self) as c:
            x, aptr, out, optr, residual, rptr = self._topk_operands(c, x, add, out, residual)
            k = self._topk_k(k, x.size)
            c.run(self.lib.byz_topk_sparsify_dev(self.ctx, x.ptr, aptr, x.size, k, optr, rptr, c.stream))
        return (out, residual, self.topk_info()) if return_info else (out, residual)

    def topk_sparsify_sharded(self, x_local, k, n_total, rank, world, add=None, all_reduce=None, out=None, residual=None,
                              return_info=False):
        """The columns layout's top-k on this rank's slice (byz_topk_sparsify_sharded_dev): rank `rank` of `world` holds
        x_local, consecutive columns of a vector of n_total, the slices in rank order; k is the global count.
        all_reduce(tensor) sums a CUDA fp64 tensor in place over the ranks on the current stream (None: one rank).  Four
        all-reduces whatever the data: 2048, 1024, 1024 and `world` doubles.  Returns this rank's (out, residual); the
        selected set is topk_sparsify's on the concatenated vector, bit for bit."""
        if not _is_device(x_local) or (add is not None and not _is_device(add)):
            raise ValueError('topk_sparsify_sharded() takes device-resident vectors')
        with _Call(self) as c:
            x, aptr, out, optr, residual, rptr = self._topk_operands(c, x_local, add, out, residual)
            n, n_total, rank, world = x.size, int(n_total), int(rank), int(world)
            if world < 1 or not 0 <= rank < world or n > n_total:
                raise ValueError('rank %d of %d with %d of %d columns' % (rank, world, n, n_total))
            k = self._topk_k(k, n_total)
            callback = self._allreduce_callback(all_reduce)
            c.run(self.lib.byz_topk_sparsify_sharded_dev(self.ctx, x.ptr, aptr, n, n_total, k, rank, world,
                                                         ctypes.cast(callback, ctypes.c_void_p), None, optr, rptr, c.stream))
        return (out, residual, self.topk_info()) if return_info else (out, residual)

    def sparsefed(self, g, k, clip=10.0, residual=None, return_info=False):
        """One round of SparseFed: agg = centered_clip(g, tau=clip, iters=1) (the norm-clipped mean: every row scaled to norm
        `clip` at most, rows with a non-finite entry excluded and still counted in the divisor), W = residual + agg, the k
        columns of W first in topk_sparsify's order are the step, the rest stay in the memory.  Returns (out, residual);
        `residual` is the caller's memory W, updated IN PLACE when given (a writable float32 numpy vector for a host g, a
        device-resident one for a device g); None is a zero memory and a fresh one comes back.  One library call.
        return_info=True also returns topk_info() with centered_clip_info()'s clipped_rows and excluded_rows."""
        params = _native.SparsefedParams(float(clip), 0)
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            params.k = self._topk_k(k, d)
            if residual is not None and _is_device(residual):
                raise ValueError('a host matrix takes a host memory (a float32 numpy vector)')
            res = self._host_f32(residual, d, writable=True) if residual is not None else np.zeros(d, dtype=np.float32)
            out = np.empty(d, dtype=np.float32)
            _check(self.lib.byz_sparsefed_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(res), _hp(out)))
            res = residual if residual is not None else res       # the caller's own array
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                d = dm.cols
                params.k = self._topk_k(k, d)
                if residual is not None:
                    res, rptr = residual, c.written(residual, d, 'residual').ptr
                elif dm.torch_like is not None:
                    res = _torch().zeros(d, dtype=_torch().float32, device=dm.torch_like.device)
                    rptr = res.data_ptr()
                else:
                    res = self.to_device(np.zeros(d, dtype=np.float32))      # (the caller's from here on: no temporary)
                    rptr = res.ptr
                out, optr = c.out(d)
                c.run(self.lib.byz_sparsefed_dev(self.ctx, dm.ptr, dm.rows, d, dm.ld, ctypes.byref(params), rptr, optr, c.stream))
        if not return_info:
            return out, res
        info = self.topk_info()
        info['clipped_rows'], info['excluded_rows'] = self.centered_clip_info()
        return out, res, info

    # ---- clip and noise, "weak DP" (Sun et al. 2019; FLAME's last stage; not in the reference) ----
    @staticmethod
    def _noise_params(sigma, seed, round, column_offset):
        """byz_noise_params; sigma must be finite and >= 0, seed and round are taken modulo 2^64, column_offset >= 0."""
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma >= 0.0):
            raise ValueError('sigma = %r must be finite and >= 0' % (sigma,))
        if int(column_offset) < 0:
            raise ValueError('column_offset = %r must be >= 0' % (column_offset,))
        mask = (1 << 64) - 1
        return _native.NoiseParams(sigma, int(seed) & mask, int(round) & mask, int(column_offset))

    def noise_words(self, n, seed=0, round=0, column_offset=0, like=None):
        """The n raw 32-bit words of the Philox4x32-10 stream at the global columns column_offset .. column_offset + n - 1
        (key = seed, counter = (column >> 2, round), word column & 3 of the block), as a uint32 numpy array; `like`: a torch
        CUDA tensor, for a device-resident int32 tensor with the same bits on its stream instead."""
        params = self._noise_params(0.0, seed, round, column_offset)
        n = int(n)
        with _Call(self) as c:
            if like is not None:
                c.beside(like)
            out, ptr = c.out(max(n, 0), np.int32) if like is not None else c.out(max(n, 1), np.uint32)
            c.run(self.lib.byz_noise_words_dev(self.ctx, ctypes.byref(params), n, ptr, c.stream))
            return out if like is not None else c.numpy(out)

    def gaussian_noise(self, x, sigma, seed=0, round=0, column_offset=0, scale=None, out=None):
        """out[c] = fl32((double)x[c] + sigma_eff * z[column_offset + c]): z the fp64 Box-Muller normals of the Philox stream
        addressed by GLOBAL column (include/byzagg.h), so a slice with its offset gets the whole vector's noise.  sigma_eff =
        sigma, or sigma * scale[0] with `scale` a device-resident fp64 scalar read by the kernel (no synchronisation).
        numpy in -> numpy out; device-resident x -> device-resident out.  out: a device vector to write, which may be x
        itself (in place).  sigma = 0 with no scale returns x's bits."""
        params = self._noise_params(sigma, seed, round, column_offset)
        if not _is_device(x):
            if scale is not None or out is not None:
                raise ValueError('a host vector takes neither a device scale nor an output vector')
            xh = self._host_f32(x)
            oh = np.empty(xh.size, dtype=np.float32)
            _check(self.lib.byz_gaussian_noise_host(self.ctx, _hp(xh), xh.size, ctypes.byref(params), _hp(oh)))
            return oh
        with _Call(self) as c:
            x = c.operand(x, np.float32, _f32(None), convert=False, leads=True)
            sptr = None if scale is None else c.operand(scale, np.float64, _F64, 1).ptr
            out, optr = c.out(x.size) if out is None else (out, c.written(out, x.size, 'out').ptr)
            c.run(self.lib.byz_gaussian_noise_dev(self.ctx, x.ptr, x.size, ctypes.byref(params), sptr, optr, c.stream))
        return out

    def weak_dp_info(self):
        """{clipped_rows, excluded_rows, clip} of the last clip_scales or weak_dp on this engine (synchronises)."""
        return dict(zip(('clipped_rows', 'excluded_rows', 'clip'),
                        self._read(self.lib.byz_weak_dp_info, [ctypes.c_int64, ctypes.c_int64, ctypes.c_double])))

    def clip_scales(self, sq, clip=10.0, adaptive=False, return_clip=False):
        """The clipping scales from the rows' fp64 squared norms (row_sqdist with a zero centre): d = sqrt(sq), s = 1 (d <=
        clip), clip / d (clip < d < inf), 0 (sq not finite: excluded, still counted in n).  adaptive=True takes clip =
        np.median of the finite norms (0 when there is none, and then every scale is 0).  fp64 out where sq lives: a torch
        tensor, a DeviceBuffer, or numpy for a host sq.  return_clip=True returns (scales, clip), the clip a one-element
        array of the same kind (device-resident: what gaussian_noise takes as `scale`)."""
        if not _is_device(sq):
            sq = np.ascontiguousarray(sq, dtype=np.float64)
        params = _native.WeakDpParams(float(clip), 0.0, 1 if adaptive else 0, 0, 0, 0)
        with _Call(self) as c:
            q = c.operand(sq, np.float64, _F64, leads=True)
            scales, sptr = c.out(q.size, np.float64)
            used, cptr = c.out(1, np.float64)
            c.run(self.lib.byz_clip_scales_dev(self.ctx, q.ptr, q.size, ctypes.byref(params), sptr, cptr, c.stream))
            return c.result((scales, used)) if return_clip else c.result(scales)

    def weak_dp(self, g, clip=10.0, sigma=0.01, adaptive=False, seed=0, round=0, column_offset=0, return_info=False):
        """Clip and noise: every row scaled to norm `clip` at most, the mean (centered_clip from zero with one iteration: its
        bits before the noise; rows with a non-finite entry excluded and still counted in the divisor), then gaussian_noise
        in place with standard deviation sigma.  adaptive=True is FLAME's: clip = the median of the finite rows' norms and
        the noise's standard deviation sigma * clip, read on the device.  One library call, nothing synchronises.
        return_info=True also returns weak_dp_info()."""
        noise = self._noise_params(sigma, seed, round, column_offset)
        params = _native.WeakDpParams(float(clip), noise.sigma, 1 if adaptive else 0, noise.seed, noise.round, noise.column_offset)
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            out = np.empty(d, dtype=np.float32)
            _check(self.lib.byz_weak_dp_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(out)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                out, optr = c.out(dm.cols)
                c.run(self.lib.byz_weak_dp_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params), optr, c.stream))
        return (out, self.weak_dp_info()) if return_info else out

    # ---- FLAME (Nguyen et al., USENIX Security 2022; not in the reference) ----
    def cosine_distances(self, g):
        """The pairwise COSINE distances of g's rows as a `Distances` handle, resident on the GPU: c_ij = max(0, 1 - g_ij /
        (sqrt(g_ii) sqrt(g_jj))) from the fp64 Gram, rounded once to float32; the diagonal is +inf (pairwise_distances'
        convention), a zero or non-finite row's whole row and column are +inf; symmetric bit for bit.  Up to 16,384 rows."""
        with _Call(self) as c:
            m = c.matrix(g)
            dist = DeviceBuffer(self, (m.rows, m.rows), np.float32)
            c.run(self.lib.byz_cosine_distances_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, dist.ptr, c.stream))
            self.check(c.stream)
        return Distances(dist, m.rows)

    def cosine_from_gram(self, gram, n=None, stream=None):
        """cosine_distances' second half on an (all-reduced) fp64 Gram, n x n, on the device -> `Distances`."""
        n = int(gram.shape[0]) if n is None else int(n)
        if _is_torch(gram) and (gram.dtype != _torch().float64 or not gram.is_contiguous() or not gram.is_cuda):
            raise ValueError('the Gram must be a contiguous float64 CUDA tensor')
        with _Call(self, stream) as c:
            gram = c.as_it_lies(gram)
            dist = Distances(DeviceBuffer(self, (n, n), np.float32), n)
            c.run(self.lib.byz_cosine_from_gram_dev(self.ctx, gram.ptr, n, dist.ptr, c.stream))
            self.synchronize(c.stream)
        return dist

    @staticmethod
    def _flame_sizes(n, min_samples, min_cluster_size):
        """(ms, m) checked as the library checks them (the refusals that need no GPU)."""
        n, ms = int(n), int(min_samples)
        m = n // 2 + 1 if min_cluster_size is None else int(min_cluster_size)
        if n > 16384:
            raise NotImplementedError('flame: at most 16384 rows, got %d' % n)
        if n < 2 or m < 2 or m > n or 2 * m <= n:
            raise ValueError('flame: min_cluster_size = %d must lie in 2..n and exceed n / 2 (n = %d)' % (m, n))
        if ms > 32:
            raise NotImplementedError('flame: min_samples = %d beyond 32' % ms)
        if ms < 0 or ms > n - 1:
            raise ValueError('flame: min_samples = %d outside 0..n - 1 (n = %d)' % (ms, n))
        return ms, m

    def flame_info(self):
        """{admitted, broken_rows, w_star, clip} of the last flame_select or flame on this engine (synchronises): the rows
        admitted, the rows without a finite off-diagonal distance, the threshold (+inf: nobody) and the median norm."""
        return dict(zip(('admitted', 'broken_rows', 'w_star', 'clip'),
                        self._read(self.lib.byz_flame_info, [ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double])))

    def flame_core_distances(self, distances, min_samples=1):
        """flame_select's first step alone: the min_samples-th smallest off-diagonal entry of every row (order: the distance,
        -0.0 as +0.0 and a NaN behind +inf, then the column; min_samples = 0: zeros), as a float32 numpy array."""
        if isinstance(distances, dict):
            raise ValueError('flame_core_distances() takes a Distances handle or a dense matrix')
        with _Call(self) as c:
            d, _ = c.distances(distances)
            ms, _ = self._flame_sizes(d.n, min_samples, d.n)
            core = DeviceBuffer(self, (d.n,), np.float32)
            c.run(self.lib.byz_flame_core_distances_dev(self.ctx, d.ptr, d.n, ms, core.ptr, None))
            return core.numpy()

    def flame_select(self, distances, min_samples=1, min_cluster_size=None, on_device=False, like=None):
        """FLAME's clustering on a distance matrix (a `Distances` handle or a dense symmetric matrix, diagonal +inf; cosine
        or any other): HDBSCAN with min_cluster_size m > n / 2 (default n // 2 + 1), which is one threshold on a minimum
        spanning tree of the mutual reachability graph (include/byzagg.h).  min_samples is the `hdbscan` package's;
        scikit-learn's is one more.  Returns (rows, info): the admitted rows ascending (on_device=True: the 0 / 1 int32
        flags instead, as a DeviceBuffer, or as a torch tensor beside `like`, a torch CUDA tensor) and {admitted, broken_rows,
        w_star}."""
        if isinstance(distances, dict):
            raise ValueError('flame_select() takes a Distances handle or a dense matrix')
        with _Call(self) as c:
            d, _ = c.distances(distances)
            ms, m = self._flame_sizes(d.n, min_samples, min_cluster_size)
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            flags, fptr = c.out(d.n, np.int32)
            c.run(self.lib.byz_flame_select_dev(self.ctx, d.ptr, d.n, m, ms, fptr, None))
            info = self.flame_info()
        info.pop('clip')
        return (flags if on_device else np.flatnonzero(flags.numpy()).astype(np.int64)), info

    def flame(self, g, lam=0.001, min_samples=1, min_cluster_size=None, seed=0, round=0, column_offset=0, distances=None,
              return_info=False):
        """FLAME in one library call: cosine_distances (or `distances`, which replaces that stage), flame_select, every
        admitted row clipped to the median norm of ALL rows, their mean over the admitted count, then gaussian_noise in
        place with standard deviation lam * clip, everything read on the device.  Nobody admitted: the zero vector plus the
        noise.  lam = 0: the clipped mean's bits.  return_info=True also returns {admitted_rows (ascending), admitted,
        broken_rows, w_star, clip}."""
        noise = self._noise_params(lam, seed, round, column_offset)
        dm = self._device_matrix(g)
        n = dm.rows if dm is not None else self._host_matrix(g).shape[0]
        ms, m = self._flame_sizes(n, min_samples, min_cluster_size)
        params = _native.FlameParams(noise.sigma, ms, m, noise.seed, noise.round, noise.column_offset)
        if isinstance(distances, dict):
            raise ValueError('flame() takes a Distances handle or a dense matrix as `distances`')
        with _Call(self) as c:
            dist = None
            if distances is not None:
                dist, _ = c.distances(distances)
                if dist.n != n:
                    raise ValueError('the distance matrix has %d rows, the gradients %d' % (dist.n, n))
            if dm is None:
                h = self._host_matrix(g)
                d = h.shape[1]
                out = np.empty(d, dtype=np.float32)
                flags = np.zeros(n, dtype=np.int32)
                dist_host = np.ascontiguousarray(dist.numpy(), dtype=np.float32) if dist is not None else None
                _check(self.lib.byz_flame_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(dist_host), _hp(out), _hp(flags)))
            else:
                dm = c.matrix(dm)
                out, optr = c.out(dm.cols)
                flags, fptr = c.out(n, np.int32, want=return_info)
                c.run(self.lib.byz_flame_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params),
                                             dist.ptr if dist is not None else None, optr, fptr, c.stream))
                self.check(c.stream)      # (a kernel of the Gram can only flag a failure)
                if return_info:
                    flags = _to_host(flags) if _is_torch(flags) else flags.numpy()
        if not return_info:
            return out
        info = self.flame_info()
        info['admitted_rows'] = np.flatnonzero(flags).astype(np.int64)
        return out, info

    # ---- agglomerative clustering and ClippedClustering (Li, Ngai & Voigt 2023; not in the reference) ----
    _LINKAGE_METHODS = {'average': 0, 'complete': 1, 'single': 2}

    @classmethod
    def _linkage_args(cls, n, method, fill):
        """(method code, fill) checked as the library checks them (the refusals that need no GPU)."""
        n, fill = int(n), float(fill)
        if n > 16384:
            raise NotImplementedError('linkage: at most 16384 rows, got %d' % n)
        if n < 2:
            raise ValueError('linkage: at least 2 rows, got %d' % n)
        if method not in cls._LINKAGE_METHODS:
            raise ValueError('linkage: method = %r is none of %s' % (method, ', '.join(sorted(cls._LINKAGE_METHODS))))
        if not (np.isfinite(fill) and fill >= 0.0):
            raise ValueError('linkage: fill = %r must be finite and >= 0' % fill)
        return cls._LINKAGE_METHODS[method], fill

    def linkage_info(self):
        """{merges, rescans, max_rescans} of the last linkage on this engine, ClippedClustering's included (synchronises): the
        steps, the nearest-partner caches rebuilt from a row of the working matrix, and the most of them in one step."""
        return dict(zip(('merges', 'rescans', 'max_rescans'),
                        self._read(self.lib.byz_linkage_info, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64])))

    def linkage_merges(self, distances, method='average', fill=2.0):
        """The device's merges as they are (include/byzagg.h): (pair (u - 1, 2) int32 slots a < b, height (u - 1) float64,
        size (u - 1) int32, usable (n) bool) for the u usable rows of a `Distances` handle or a dense symmetric matrix."""
        if isinstance(distances, dict):
            raise ValueError('linkage() takes a Distances handle or a dense matrix')
        with _Call(self) as c:
            d, _ = c.distances(distances)
            code, fill = self._linkage_args(d.n, method, fill)
            pair = DeviceBuffer(self, (d.n - 1, 2), np.int32)
            height = DeviceBuffer(self, (d.n - 1,), np.float64)
            size = DeviceBuffer(self, (d.n - 1,), np.int32)
            usable = DeviceBuffer(self, (d.n,), np.int32)
            c.run(self.lib.byz_linkage_dev(self.ctx, d.ptr, d.n, code, ctypes.byref(ctypes.c_double(fill)), pair.ptr, height.ptr,
                                           size.ptr, usable.ptr, None))
            usable = usable.numpy() != 0
            merges = max(int(usable.sum()) - 1, 0)
            return pair.numpy()[:merges], height.numpy()[:merges], size.numpy()[:merges], usable

    def linkage(self, distances, method='average', fill=2.0):
        """Agglomerative clustering of a distance matrix (a `Distances` handle or a dense symmetric matrix, the diagonal
        ignored; cosine, Euclidean, Manhattan or any other) with 'average', 'complete' or 'single' linkage, on the GPU.
        Returns (Z, usable): Z is scipy's (u - 1) x 4 float64 linkage matrix over the u usable rows -- the rows with a finite
        off-diagonal distance, `usable` their mask; observation i of Z is the i-th usable row -- built on the host from the
        device's merges, so scipy.cluster.hierarchy.fcluster and dendrogram take it.  An entry between usable rows that is
        not finite or is negative counts as `fill`.  Merges are made in the order (distance, lower row, higher row), which
        fixes every tie; the heights are scipy's up to the rounding of a different merge order."""
        pair, height, size, usable = self.linkage_merges(distances, method=method, fill=fill)
        u = int(usable.sum())
        ident = np.full(usable.size, -1, dtype=np.int64)      # the scipy id of the cluster a slot holds
        ident[usable] = np.arange(u)
        z = np.zeros((max(u - 1, 0), 4), dtype=np.float64)
        for t in range(z.shape[0]):
            a, b = int(pair[t, 0]), int(pair[t, 1])
            lo, hi = sorted((ident[a], ident[b]))
            z[t] = (lo, hi, height[t], size[t])
            ident[a] = u + t
        return z, usable

    def linkage_cut(self, pair, usable, n_clusters):
        """The cut of linkage_merges' `pair` into n_clusters: (labels (n) int32, the clusters numbered by their lowest row in
        ascending order and -1 for a row that is not usable, sizes (n_clusters) int32)."""
        usable = np.ascontiguousarray(np.asarray(usable) != 0, dtype=np.int32)
        n, c_count = int(usable.size), int(n_clusters)
        if n > 16384:
            raise NotImplementedError('linkage_cut: at most 16384 rows, got %d' % n)
        if n < 2 or c_count < 1 or c_count > n:
            raise ValueError('linkage_cut: %d clusters of %d rows (at least 2 rows, 1..n clusters)' % (c_count, n))
        merges = np.full((n - 1, 2), -1, dtype=np.int32)
        pair = np.asarray(pair, dtype=np.int32).reshape(-1, 2)
        if pair.shape[0] > n - 1:
            raise ValueError('linkage_cut: %d merges of %d rows' % (pair.shape[0], n))
        merges[:pair.shape[0]] = pair
        with _Call(self) as c:
            p, f = c.upload(merges), c.upload(usable)
            labels = DeviceBuffer(self, (n,), np.int32)
            sizes = DeviceBuffer(self, (c_count,), np.int32)
            c.run(self.lib.byz_linkage_cut_dev(self.ctx, p.ptr, n, f.ptr, c_count, labels.ptr, sizes.ptr, None))
            return labels.numpy(), sizes.numpy()

    def clipped_clustering_info(self):
        """{admitted, usable, top_height, second_height, clip} of the last clipped_clustering_select or clipped_clustering on
        this engine (synchronises): the rows admitted, the rows with a finite off-diagonal distance, the heights of the
        last merge and of the one before (0 where there is none) and the clip used (0 after a selection alone)."""
        return dict(zip(('admitted', 'usable', 'top_height', 'second_height', 'clip'),
                        self._read(self.lib.byz_clipped_clustering_info,
                                   [ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double])))

    def clipped_clustering_select(self, distances, method='average', fill=2.0, on_device=False, like=None):
        """ClippedClustering's selection on a distance matrix: the linkage, the cut into two clusters and the LARGER one
        (equal sizes: the cluster of the lowest usable row).  Returns (rows, info): the admitted rows ascending
        (on_device=True: the 0 / 1 int32 flags instead, as a DeviceBuffer, or a torch tensor beside `like`) and {admitted,
        usable, top_height, second_height}."""
        if isinstance(distances, dict):
            raise ValueError('clipped_clustering_select() takes a Distances handle or a dense matrix')
        with _Call(self) as c:
            d, _ = c.distances(distances)
            code, fill = self._linkage_args(d.n, method, fill)
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            flags, fptr = c.out(d.n, np.int32)
            c.run(self.lib.byz_clipped_clustering_select_dev(self.ctx, d.ptr, d.n, code, ctypes.byref(ctypes.c_double(fill)), fptr,
                                                             None))
            info = self.clipped_clustering_info()
        info.pop('clip')
        return (flags if on_device else np.flatnonzero(flags.numpy()).astype(np.int64)), info

    def clipped_clustering(self, g, clip=None, method='average', fill=2.0, distances=None, sq=None, return_info=False):
        """ClippedClustering in one library call: cosine_distances (or `distances`, which replaces that stage),
        clipped_clustering_select, every admitted row clipped to `clip` (None: the median norm of this round's finite rows,
        read on the device), their mean over the admitted count.  `sq`: the rows' fp64 squared norms where the caller has
        them (device-resident for a device matrix), which spares the pass that computes them.  Nobody admitted: the zero
        vector.  return_info=True also returns {admitted_rows (ascending), admitted, usable, top_height, second_height,
        clip}."""
        dm = self._device_matrix(g)
        n = dm.rows if dm is not None else self._host_matrix(g).shape[0]
        code, fill = self._linkage_args(n, method, fill)
        if clip is not None and not float(clip) > 0.0:
            raise ValueError('clipped_clustering: clip = %r must be > 0 (None: the median norm)' % clip)
        params = _native.ClippedClusteringParams(0.0 if clip is None else float(clip), 1 if clip is None else 0, code, fill)
        if isinstance(distances, dict):
            raise ValueError('clipped_clustering() takes a Distances handle or a dense matrix as `distances`')
        with _Call(self) as c:
            dist = None
            if distances is not None:
                dist, _ = c.distances(distances)
                if dist.n != n:
                    raise ValueError('the distance matrix has %d rows, the gradients %d' % (dist.n, n))
            if dm is None:
                h = self._host_matrix(g)
                d = h.shape[1]
                out = np.empty(d, dtype=np.float32)
                flags = np.zeros(n, dtype=np.int32)
                dist_host = np.ascontiguousarray(dist.numpy(), dtype=np.float32) if dist is not None else None
                sq_host = None if sq is None else np.ascontiguousarray(_to_host(sq), dtype=np.float64).reshape(-1)
                if sq_host is not None and sq_host.size != n:
                    raise ValueError('expected %d squared norms, got %d' % (n, sq_host.size))
                _check(self.lib.byz_clipped_clustering_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(dist_host),
                                                            _hp(sq_host), _hp(out), _hp(flags)))
            else:
                dm = c.matrix(dm)
                q = None if sq is None else c.operand(sq, np.float64, _F64, n)
                out, optr = c.out(dm.cols)
                flags, fptr = c.out(n, np.int32, want=return_info)
                c.run(self.lib.byz_clipped_clustering_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params),
                                                          dist.ptr if dist is not None else None,
                                                          q.ptr if q is not None else None, optr, fptr, c.stream))
                self.check(c.stream)      # (a kernel of the Gram can only flag a failure)
                if return_info:
                    flags = _to_host(flags) if _is_torch(flags) else flags.numpy()
        if not return_info:
            return out
        info = self.clipped_clustering_info()
        info['admitted_rows'] = np.flatnonzero(flags).astype(np.int64)
        return out, info

    # ---- FABA (Xia, Chen, Yu & Ma, IJCAI 2019; not in the reference) ----
    @staticmethod
    def _faba_args(n, remove_count, power=2):
        """(remove_count, power) checked as the library checks them (the refusals that need no GPU)."""
        n, r = int(n), int(remove_count)
        if n > 16384:
            raise NotImplementedError('faba: at most 16384 rows, got %d' % n)
        if n < 2:
            raise ValueError('faba: at least 2 rows, got %d' % n)
        if r < 0 or r > n - 1:
            raise ValueError('faba: remove_count = %d outside 0..n - 1 (n = %d)' % (r, n))
        if power not in (1, 2):
            raise ValueError('faba: power = %r is neither 1 (the distances) nor 2 (their squares)' % (power,))
        return r, int(power)

    def faba_info(self):
        """{removed, kept, forced, last_score, divisor} of the last faba_select or faba on this engine (synchronises): the rows
        removed and kept, the rows removed beyond remove_count because a row had an unusable distance to a kept row, the
        summed (squared) distance of the last removed row at its removal (0: nobody was removed) and the sum's divisor."""
        return dict(zip(('removed', 'kept', 'forced', 'last_score', 'divisor'),
                        self._read(self.lib.byz_faba_info,
                                   [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double])))

    def faba_select(self, distances, remove_count, power=2, on_device=False, like=None, return_order=False):
        """FABA's selection on a distance matrix (a `Distances` handle or a dense symmetric matrix, the diagonal ignored):
        remove_count times, the kept row with the largest sum of (power 2: squared) distances to the kept rows is removed,
        which for Euclidean distances is the row farthest from the kept rows' mean (include/byzagg.h states the rule).  A
        row with an entry that is not finite or is negative against a kept row goes first and is never kept.  power=1 sums
        the distances themselves (cosine, Manhattan).  Returns (rows, info): the kept rows ascending (on_device=True: the
        0 / 1 int32 flags instead, as a DeviceBuffer, or a torch tensor beside `like`) and {removed, kept, forced,
        last_score, divisor}; return_order=True: (rows, order, info), order the removed rows in removal order (on_device:
        n int32, -1 behind them)."""
        if isinstance(distances, dict):
            raise ValueError('faba_select() takes a Distances handle or a dense matrix')
        with _Call(self) as c:
            d, _ = c.distances(distances)
            r, power = self._faba_args(d.n, remove_count, power)
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            flags, fptr = c.out(d.n, np.int32)
            order, optr = c.out(d.n, np.int32, want=return_order)
            c.run(self.lib.byz_faba_select_dev(self.ctx, d.ptr, d.n, r, power, fptr, optr, None))
            info = self.faba_info()
        if not on_device:
            flags = np.flatnonzero(flags.numpy()).astype(np.int64)
            if return_order:
                order = order.numpy()[:info['removed']].astype(np.int64)
        return (flags, order, info) if return_order else (flags, info)

    def faba(self, g, users_count, corrupted_count, distances=None, return_info=False):
        """FABA in one library call: pairwise_distances (or `distances`, which replaces that stage), faba_select with
        remove_count = corrupted_count on the squared distances, and the mean of the kept rows: scaled_rows_sum's bits with
        the 0 / 1 flags as weights and the kept count, read on the device, as the divisor.  Nobody kept: the zero vector.
        return_info=True also returns {kept_rows (ascending), order (the removed rows in removal order), removed, kept,
        forced, last_score, divisor}."""
        dm = self._device_matrix(g)
        n = dm.rows if dm is not None else self._host_matrix(g).shape[0]
        r, _ = self._faba_args(n, corrupted_count)
        if isinstance(distances, dict):
            raise ValueError('faba() takes a Distances handle or a dense matrix as `distances`')
        with _Call(self) as c:
            dist = None
            if distances is not None:
                dist, _ = c.distances(distances)
                if dist.n != n:
                    raise ValueError('the distance matrix has %d rows, the gradients %d' % (dist.n, n))
            if dm is None:
                h = self._host_matrix(g)
                d = h.shape[1]
                out = np.empty(d, dtype=np.float32)
                flags = np.zeros(n, dtype=np.int32)
                order = np.full(n, -1, dtype=np.int32)
                dist_host = np.ascontiguousarray(dist.numpy(), dtype=np.float32) if dist is not None else None
                _check(self.lib.byz_faba_host(self.ctx, _hp(h), n, d, r, _hp(dist_host), _hp(out), _hp(flags), _hp(order)))
            else:
                dm = c.matrix(dm)
                out, optr = c.out(dm.cols)
                flags, fptr = c.out(n, np.int32, want=return_info)
                order, rptr = c.out(n, np.int32, want=return_info)
                c.run(self.lib.byz_faba_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, r, dist.ptr if dist is not None else None,
                                            optr, fptr, rptr, c.stream))
                self.check(c.stream)      # (a kernel of the Gram can only flag a failure)
                if return_info:
                    flags = _to_host(flags) if _is_torch(flags) else flags.numpy()
                    order = _to_host(order) if _is_torch(order) else order.numpy()
        if not return_info:
            return out
        info = self.faba_info()
        info['kept_rows'] = np.flatnonzero(flags).astype(np.int64)
        info['order'] = np.asarray(order)[:info['removed']].astype(np.int64)
        return out, info

    # ---- AFA (Munoz-Gonzalez, Co & Lupu, arXiv:1909.05125; not in the reference) ----
    @staticmethod
    def _afa_params(n, xi, delta_xi, max_rounds):
        """byz_afa_params, checked as the library checks them (the refusals that need no GPU)."""
        n = int(n)
        if n > 16384:
            raise NotImplementedError('afa: at most 16384 rows, got %d' % n)
        if n < 2:
            raise ValueError('afa: at least 2 rows, got %d' % n)
        xi, delta_xi, max_rounds = float(xi), float(delta_xi), int(0 if max_rounds is None else max_rounds)
        if not (np.isfinite(xi) and xi >= 0.0 and np.isfinite(delta_xi) and delta_xi >= 0.0) or max_rounds < 0:
            raise ValueError('afa: xi = %r and delta_xi = %r must be finite and >= 0, max_rounds = %r >= 0' % (xi, delta_xi, max_rounds))
        return _native.AfaParams(xi, delta_xi, max_rounds)

    def afa_info(self):
        """{rounds, kept, removed, excluded, branch, degenerate, mean, med, sd, thr, divisor} of the last afa_select or afa on
        this engine (synchronises): the rounds run, the rows kept, removed by a round and excluded before the first, the side
        of the last removing round (-1 below the median, +1 above, 0: nobody was removed), whether a round's A was not > 0,
        the last complete round's statistics and the kept rows' weights summed."""
        counts, stats, divisor = (ctypes.c_int64 * 6)(), (ctypes.c_double * 4)(), ctypes.c_double()
        _check(self.lib.byz_afa_info(self.ctx, counts, stats, ctypes.byref(divisor)))
        self._unsynced.discard(self._last)
        info = dict(zip(('rounds', 'kept', 'removed', 'excluded', 'branch', 'degenerate'), (int(v) for v in counts)))
        info.update(zip(('mean', 'med', 'sd', 'thr'), (float(v) for v in stats)))
        info['degenerate'] = bool(info['degenerate'])
        info['divisor'] = divisor.value
        return info

    def afa_select(self, gram, weights=None, xi=2.0, delta_xi=0.5, max_rounds=None, on_device=False, like=None):
        """AFA's selection on an fp64 Gram (n x n, as `gram` returns it; taken as symmetric): every row's cosine with the
        weighted sum of the rows still kept, the rows more than xi standard deviations from the median removed on the side the
        mean points away from, xi raised by delta_xi, until a round removes nobody (include/byzagg.h states the rule).  A row
        whose diagonal entry or weight is not finite and positive is excluded before the first round.  Returns (rows, info):
        the kept rows ascending (on_device=True: the 0 / 1 int32 flags instead, as a DeviceBuffer, or a torch tensor beside
        `like`) and afa_info()'s fields with `round_of` (int32: the round that removed a row, 0 excluded, -1 kept) and `score`
        (fp64: the last cosine a row had), host arrays unless on_device."""
        with _Call(self) as c:
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            shape = tuple(gram.shape)
            if len(shape) != 2 or shape[0] != shape[1]:
                raise ValueError('afa_select() takes a square fp64 Gram, got shape %r' % (shape,))
            n = shape[0]
            params = self._afa_params(n, xi, delta_xi, max_rounds)
            gm = c.operand(gram, np.float64, _F64, n * n)
            w = c.operand(weights, np.float64, _F64, n) if weights is not None else None
            flags, fptr = c.out(n, np.int32)
            round_of, rptr = c.out(n, np.int32)
            score, sptr = c.out(n, np.float64)
            c.run(self.lib.byz_afa_select_dev(self.ctx, gm.ptr, n, w.ptr if w is not None else None, ctypes.byref(params), fptr, rptr,
                                              sptr, c.stream))
            info = self.afa_info()
        if not on_device:
            flags = np.flatnonzero(flags.numpy()).astype(np.int64)
            round_of, score = round_of.numpy(), score.numpy()
        info['round_of'], info['score'] = round_of, score
        return flags, info

    def afa(self, g, users_count=None, corrupted_count=None, weights=None, xi=2.0, delta_xi=0.5, max_rounds=None, gram=None,
            return_info=False):
        """AFA in one library call: gram (or `gram`, which replaces that stage), afa_select, and the weighted mean of the kept
        rows: scaled_rows_sum's bits with the weights w_k * kept_k and their sum, read on the device, as the divisor.  Nobody
        kept: the zero vector.  users_count and corrupted_count are accepted and unused: the rule needs no count.
        return_info=True also returns afa_info()'s fields with kept_rows (ascending), excluded_rows, round_of and score."""
        dm = self._device_matrix(g)
        n = dm.rows if dm is not None else self._host_matrix(g).shape[0]
        params = self._afa_params(n, xi, delta_xi, max_rounds)
        if gram is not None and tuple(gram.shape) != (n, n):
            raise ValueError('the Gram has shape %r, the gradients %d rows' % (tuple(gram.shape), n))
        if dm is None:
            h = self._host_matrix(g)
            d = h.shape[1]
            out = np.empty(d, dtype=np.float32)
            flags, round_of, score = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64)
            w_host = np.ascontiguousarray(_to_host(weights), dtype=np.float64).ravel() if weights is not None else None
            if w_host is not None and w_host.size != n:
                raise ValueError('expected %d values, got %d' % (n, w_host.size))
            if gram is not None:
                gram = np.ascontiguousarray(gram.numpy() if isinstance(gram, DeviceBuffer) else _to_host(gram), dtype=np.float64)
            _check(self.lib.byz_afa_host(self.ctx, _hp(h), n, d, _hp(w_host), ctypes.byref(params), _hp(gram), _hp(out), _hp(flags),
                                         _hp(round_of), _hp(score)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                gm = c.operand(gram, np.float64, _F64, n * n) if gram is not None else None
                w = c.operand(weights, np.float64, _F64, n) if weights is not None else None
                out, optr = c.out(dm.cols)
                flags, fptr = c.out(n, np.int32, want=return_info)
                round_of, rptr = c.out(n, np.int32, want=return_info)
                score, sptr = c.out(n, np.float64, want=return_info)
                c.run(self.lib.byz_afa_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, w.ptr if w is not None else None,
                                           ctypes.byref(params), gm.ptr if gm is not None else None, optr, fptr, rptr, sptr, c.stream))
                self.check(c.stream)      # (a kernel of the Gram can only flag a failure)
                if return_info:
                    flags, round_of, score = (_to_host(v) if _is_torch(v) else v.numpy() for v in (flags, round_of, score))
        if not return_info:
            return out
        info = self.afa_info()
        round_of = np.asarray(round_of)
        info.update(kept_rows=np.flatnonzero(flags).astype(np.int64), excluded_rows=np.flatnonzero(round_of == 0).astype(np.int64),
                    round_of=round_of, score=np.asarray(score))
        return out, info

    # ---- Auror (Shen, Tople & Saxena, ACSAC 2016; not in the reference) ----
    @staticmethod
    def _auror_params(n, alpha, tau=0.5, max_iter=32, accumulate=False):
        """byz_auror_params, checked as the library checks them (the refusals that need no GPU)."""
        n = int(n)
        if n > 16384:
            raise NotImplementedError('auror: at most 16384 rows, got %d' % n)
        if n < 1:
            raise ValueError('auror: at least 1 row, got %d' % n)
        alpha, tau, max_iter = float(alpha), float(tau), int(max_iter)
        if not (np.isfinite(alpha) and alpha >= 0.0 and 0.0 <= tau <= 1.0) or max_iter < 1:
            raise ValueError('auror: alpha = %r must be finite and >= 0, 0 <= tau = %r <= 1, max_iter = %r >= 1' % (alpha, tau, max_iter))
        return _native.AurorParams(alpha, tau, max_iter, 1 if accumulate else 0)

    def auror_info(self):
        """{indicative, removed, kept, bad_rows, capped_cols} of the last auror_select or auror on this engine (synchronises):
        the indicative columns the selection read (accumulated: over the rounds), the rows removed (bad rows included) and
        kept, the rows with a non-finite value, the columns max_iter stopped."""
        return dict(zip(('indicative', 'removed', 'kept', 'bad_rows', 'capped_cols'),
                        self._read(self.lib.byz_auror_info, [ctypes.c_int64] * 5)))

    def _auror_history(self, c, n, votes, bad, counts):
        """The caller's votes, bad flags and counts as they lie on the device (all three or none), or fresh arrays."""
        given = [v is not None for v in (votes, bad, counts)]
        if any(given) and not all(given):
            raise ValueError('auror: votes, bad and counts come together or not at all')
        if not given[0]:
            return c.out(n, np.int64), c.out(n, np.int32), c.out(4, np.int64), False
        ops = []
        for v, dtype, count, what in ((votes, np.int64, n, 'votes'), (bad, np.int32, n, 'bad flags'), (counts, np.int64, 4, 'counts')):
            if not _is_device(v):
                raise ValueError('auror: the %s to add to must be device-resident' % what)
            op = c.operand(v, dtype, _ints(what), count, convert=False)
            ops.append((v, op.ptr))
        return ops[0], ops[1], ops[2], True

    def auror_votes(self, g, alpha, max_iter=32, votes=None, bad=None, counts=None, return_gap=False):
        """Auror's votes on a device-resident or host matrix: every column's finite values split in two by Lloyd's 2-means from
        (min, max), a column whose centres end more than alpha apart indicative, one vote for every row in the smaller cluster
        of an indicative column (include/byzagg.h states the rule).  Returns (votes int64[n], bad int32[n], counts int64[4] =
        {indicative, clustered, capped columns, 0}) and, return_gap=True, gap float64[D] (the centres' final distance, 0
        where a column was not clustered: what alpha is chosen from).  votes=, bad=, counts= (device-resident, all three): an
        earlier call's, which this call adds to in place.  Device arrays for a device matrix, numpy for a host one."""
        with _Call(self) as c:
            m = c.matrix(g)
            (v, vptr), (b, bptr), (k, kptr), add = self._auror_history(c, m.rows, votes, bad, counts)
            params = self._auror_params(m.rows, alpha, 0.5, max_iter, accumulate=add)
            gap, gptr = c.out(m.cols, np.float64, want=return_gap)
            c.run(self.lib.byz_auror_votes_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, ctypes.byref(params), vptr, bptr, kptr, gptr,
                                               c.stream))
            return c.result((v, b, k, gap) if return_gap else (v, b, k))

    def auror_select(self, votes, bad, counts, tau=0.5, on_device=False, like=None):
        """Auror's selection: row i is removed iff it is bad, or counts[0] > 0 and votes[i] > tau * counts[0].  Returns (rows,
        info): the kept rows ascending (on_device=True: the 0 / 1 int32 flags instead, as a DeviceBuffer, or a torch tensor
        beside `like`) and auror_info()'s fields."""
        with _Call(self) as c:
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            b = c.operand(bad, np.int32, _ints('bad flags'))
            n = b.size
            params = self._auror_params(n, 0.0, tau)
            v = c.operand(votes, np.int64, _ints('votes'), n)
            k = c.operand(counts, np.int64, _ints('counts'), 4)
            flags, fptr = c.out(n, np.int32)
            c.run(self.lib.byz_auror_select_dev(self.ctx, v.ptr, b.ptr, k.ptr, n, ctypes.byref(params), fptr, c.stream))
            info = self.auror_info()
        if not on_device:
            flags = np.flatnonzero(flags.numpy()).astype(np.int64)
        return flags, info

    def auror(self, g, users_count=None, corrupted_count=None, alpha=None, tau=0.5, max_iter=32, votes=None, bad=None, counts=None,
              return_info=False):
        """Auror in one library call: auror_votes, auror_select and the mean of the kept rows: scaled_rows_sum's bits with the
        0 / 1 flags as weights and the kept count, read on the device, as the divisor.  Nobody kept: the zero vector.
        users_count and corrupted_count are accepted and unused: the rule needs no count.  alpha has no default (a value below
        about 1.6 standard deviations of an honest column makes every column indicative).  votes=, bad=, counts=
        (device-resident, all three): the history this call adds to in place (device matrices only).  return_info=True also
        returns auror_info()'s fields with kept_rows (ascending), votes, bad, counts and gap as host arrays."""
        if alpha is None:
            raise ValueError('auror: alpha has no default; choose it from auror_votes(..., return_gap=True)')
        dm = self._device_matrix(g)
        n = dm.rows if dm is not None else self._host_matrix(g).shape[0]
        history = votes is not None or bad is not None or counts is not None
        params = self._auror_params(n, alpha, tau, max_iter, accumulate=history)
        if dm is None:
            if history:
                raise ValueError('auror: a history lives on the device; pass a device-resident matrix with it')
            h = self._host_matrix(g)
            d = h.shape[1]
            out = np.empty(d, dtype=np.float32)
            flags, v, b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
            k, gap = np.zeros(4, dtype=np.int64), np.zeros(d, dtype=np.float64)
            _check(self.lib.byz_auror_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(out), _hp(flags), _hp(v), _hp(b), _hp(k),
                                           _hp(gap)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                out, optr = c.out(dm.cols)
                if history:
                    (v, vptr), (b, bptr), (k, kptr), _ = self._auror_history(c, n, votes, bad, counts)
                elif return_info:
                    (v, vptr), (b, bptr), (k, kptr) = c.out(n, np.int64), c.out(n, np.int32), c.out(4, np.int64)
                else:
                    (v, vptr), (b, bptr), (k, kptr) = (None, None), (None, None), (None, None)
                flags, fptr = c.out(n, np.int32, want=return_info)
                gap, gptr = c.out(dm.cols, np.float64, want=return_info)
                c.run(self.lib.byz_auror_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params), vptr, bptr, kptr, optr,
                                             fptr, gptr, c.stream))
                if return_info:
                    flags, v, b, k, gap = (_to_host(x) if _is_torch(x) else x.numpy() for x in (flags, v, b, k, gap))
        if not return_info:
            return out
        info = self.auror_info()
        info.update(kept_rows=np.flatnonzero(flags).astype(np.int64), votes=np.asarray(v), bad=np.asarray(b), counts=np.asarray(k),
                    gap=np.asarray(gap))
        return out, info

    # ---- FoolsGold (Fung, Yoon & Beschastnikh, arXiv:1808.04866; not in the reference) ----
    @staticmethod
    def _foolsgold_params(n, kappa=1.0, normalise='count'):
        """byz_foolsgold_params, checked as the library checks them (the refusals that need no GPU)."""
        n = int(n)
        if n > 1 << 20:
            raise NotImplementedError('foolsgold: at most %d rows, got %d' % (1 << 20, n))
        if n < 1:
            raise ValueError('foolsgold: at least 1 row, got %d' % n)
        kappa = float(kappa)
        if not (np.isfinite(kappa) and kappa > 0.0):
            raise ValueError('foolsgold: kappa = %r must be finite and > 0' % kappa)
        if normalise not in FOOLSGOLD_NORMALISE:
            raise ValueError("foolsgold: normalise = %r is neither 'count' nor 'sum'" % (normalise,))
        return _native.FoolsgoldParams(kappa, FOOLSGOLD_NORMALISE[normalise])

    @staticmethod
    def _foolsgold_window(d, columns):
        """columns (None: all; a (start, stop) pair or a slice of step 1) -> (col_start, col_count) inside d columns."""
        if columns is None:
            return 0, int(d)
        if isinstance(columns, slice):
            if columns.step not in (None, 1):
                raise ValueError('foolsgold: the window is contiguous, got step %r' % (columns.step,))
            columns = (0 if columns.start is None else columns.start, d if columns.stop is None else columns.stop)
        start, stop = (int(v) for v in columns)
        if not 0 <= start < stop <= int(d):
            raise ValueError('foolsgold: the window [%d, %d) lies outside the %d columns' % (start, stop, d))
        return start, stop - start

    def _foolsgold_history(self, c, history, n, width):
        """The history as an _Operand: device-resident, n x width float32 with unit column stride (any ld)."""
        h = self._device_matrix(history)
        if h is None:
            raise ValueError('foolsgold: the history lives on the device (defences.FoolsGoldHistory owns one)')
        if h.shape != (n, width):
            raise ValueError('foolsgold: the history has shape %r, the window is %d x %d' % (h.shape, n, width))
        return c._adopt(h, False)

    def foolsgold_info(self):
        """{usable, excluded, at_zero, at_one, degenerate, top, divisor} of the last foolsgold_weights or foolsgold on this
        engine (synchronises): the rows with a finite diagonal >= 0 and the others, the usable rows whose weight is exactly 0
        and exactly 1, whether two or more usable rows all had a raw weight of 0, the largest raw weight, and T."""
        counts, stats = (ctypes.c_int64 * 5)(), (ctypes.c_double * 2)()
        _check(self.lib.byz_foolsgold_info(self.ctx, counts, stats))
        self._unsynced.discard(self._last)
        info = dict(zip(('usable', 'excluded', 'at_zero', 'at_one', 'degenerate'), (int(v) for v in counts)))
        info['degenerate'] = bool(info['degenerate'])
        info['top'], info['divisor'] = float(stats[0]), float(stats[1])
        return info

    def rows_add(self, history, g, columns=None):
        """history[i][c] = fl32(history[i][c] + g[i][col_start + c]) in place: numpy's float32 += of g's column window
        (`columns`: None for all, or (start, stop)) onto a device-resident n x w float32 matrix.  Any leading dimension and any
        4-byte base alignment on either side.  Returns `history`."""
        with _Call(self) as c:
            m = c.matrix(g)
            start, width = self._foolsgold_window(m.cols, columns)
            h = self._foolsgold_history(c, history, m.rows, width)
            c.run(self.lib.byz_rows_add_dev(self.ctx, h.ptr, h.ld, m.ptr, m.rows, width, m.ld, start, c.stream))
        return history

    def foolsgold_weights(self, gram, kappa=1.0, on_device=False, like=None):
        """FoolsGold's weights on an fp64 Gram (n x n, as `gram` returns it; taken as symmetric): every row's largest cosine
        with another row, pardoned where the other row's own maximum is larger, turned into a weight by the clipped logit
        (include/byzagg.h states the rule).  A row whose diagonal entry is not finite or is negative is excluded: weight 0.
        Returns (weights, info): n fp64 weights (on_device=True: a DeviceBuffer, or a torch tensor beside `like`) and
        foolsgold_info()'s fields with `maxcs` (m), `alpha` (a), `rescaled` (w of step 8) and `usable_flags` (int32 0 / 1), host arrays
        unless on_device.  The `divisor` reported is the usable count."""
        return self._foolsgold_weights(gram, kappa, 'count', on_device, like)

    def _foolsgold_weights(self, gram, kappa, normalise, on_device, like):
        """foolsgold_weights with the divisor's kind chosen (the columns layout reads T from it)."""
        with _Call(self) as c:
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            shape = tuple(gram.shape)
            if len(shape) != 2 or shape[0] != shape[1]:
                raise ValueError('foolsgold_weights() takes a square fp64 Gram, got shape %r' % (shape,))
            n = shape[0]
            params = self._foolsgold_params(n, kappa, normalise)
            gm = c.operand(gram, np.float64, _F64, n * n)
            outs = [c.out(n, np.float64) for _ in range(4)] + [c.out(n, np.int32)]
            (weights, wptr), (maxcs, mptr), (alpha, aptr), (rescaled, rptr), (usable, uptr) = outs
            c.run(self.lib.byz_foolsgold_weights_dev(self.ctx, gm.ptr, n, ctypes.byref(params), wptr, mptr, aptr, c.stream))
            c.run(self.lib.byz_foolsgold_trace_dev(self.ctx, n, rptr, uptr, c.stream))
            info = self.foolsgold_info()
        if not on_device:
            weights, maxcs, alpha, rescaled, usable = (v.numpy() for v in (weights, maxcs, alpha, rescaled, usable))
        info.update(maxcs=maxcs, alpha=alpha, rescaled=rescaled, usable_flags=usable)
        return weights, info

    def foolsgold(self, g, users_count=None, corrupted_count=None, history=None, columns=None, kappa=1.0, normalise='count',
                  gram=None, return_info=False):
        """FoolsGold in one library call: the history update (`history`: a device-resident n x w float32 matrix, added to in
        place; None: stateless), gram of the history -- or of g's column window without one; `gram` replaces that stage --,
        foolsgold_weights, and the weighted sum of THIS round's rows over T: scaled_rows_sum's bits with the weights and T read
        on the device.  normalise='count': T is the number of usable rows, so with every weight 1 the rule is the mean;
        'sum': T is the weights' sum.  T == 0: the zero vector.  `columns`: None for all, or (start, stop): the window of g the
        history and the Gram are taken over (the output layer, say).  users_count and corrupted_count are accepted and unused:
        the rule needs no count.  return_info=True also returns foolsgold_info()'s fields with `weights` (fp64, host)."""
        dm = self._device_matrix(g)
        n, d = (dm.rows, dm.cols) if dm is not None else self._host_matrix(g).shape
        params = self._foolsgold_params(n, kappa, normalise)
        start, width = self._foolsgold_window(d, columns)
        if gram is not None and tuple(gram.shape) != (n, n):
            raise ValueError('the Gram has shape %r, the gradients %d rows' % (tuple(gram.shape), n))
        if dm is None:
            if history is not None:
                raise ValueError('foolsgold: a history lives on the device; pass a device-resident matrix with it')
            h = self._host_matrix(g)
            out, weights = np.empty(d, dtype=np.float32), np.zeros(n, dtype=np.float64)
            if gram is not None:
                gram = np.ascontiguousarray(gram.numpy() if isinstance(gram, DeviceBuffer) else _to_host(gram), dtype=np.float64)
            _check(self.lib.byz_foolsgold_host(self.ctx, _hp(h), n, d, None, start, width, ctypes.byref(params), _hp(gram), _hp(out),
                                               _hp(weights)))
        else:
            with _Call(self) as c:
                dm = c.matrix(dm)
                hm = self._foolsgold_history(c, history, n, width) if history is not None else None
                gm = c.operand(gram, np.float64, _F64, n * n) if gram is not None else None
                out, optr = c.out(d)
                weights, wptr = c.out(n, np.float64, want=return_info)
                c.run(self.lib.byz_foolsgold_dev(self.ctx, dm.ptr, n, d, dm.ld, hm.ptr if hm is not None else None,
                                                 hm.ld if hm is not None else 0, start, width, ctypes.byref(params),
                                                 gm.ptr if gm is not None else None, optr, wptr, c.stream))
                self.check(c.stream)      # (a kernel of the Gram can only flag a failure)
                if return_info:
                    weights = _to_host(weights) if _is_torch(weights) else weights.numpy()
        if not return_info:
            return out
        info = self.foolsgold_info()
        info['weights'] = np.asarray(weights)
        return out, info

    # ---- Multi-Metrics (Huang et al., ICCV 2023; not in the reference) ----
    def manhattan_distances(self, g):
        """The pairwise MANHATTAN (L1) distances of g's rows as a `Distances` handle, resident on the GPU: m_ij = sum_c
        |g_ic - g_jc|, fp32 chains of 128 terms folded into fp64 and rounded once to float32 (relative error at most
        130 * 2^-24); the diagonal is +inf (pairwise_distances' convention), a pair whose sum is not finite is +inf, a zero
        row is an ordinary row; symmetric bit for bit.  Up to 16,384 rows.  Whatever takes `distances=` takes it."""
        with _Call(self) as c:
            m = c.matrix(g)
            if m.rows > 16384:
                raise NotImplementedError('manhattan_distances: at most 16384 rows, got %d' % m.rows)
            dist = DeviceBuffer(self, (m.rows, m.rows), np.float32)
            c.run(self.lib.byz_manhattan_distances_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, dist.ptr, c.stream))
            self.check(c.stream)
        return Distances(dist, m.rows)

    def manhattan_sums(self, g):
        """manhattan_distances' first half: the n x n fp64 sums over the columns of a device-resident slice (additive over
        column slices: the columns layout all-reduces them)."""
        with _Call(self) as c:
            m = c.matrix(g, needs='manhattan_sums')
            out, ptr = c.out((m.rows, m.rows), np.float64)
            c.run(self.lib.byz_manhattan_sums_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, ptr, c.stream))
        return out

    def manhattan_from_sums(self, sums, n=None, stream=None):
        """manhattan_distances' second half on (all-reduced) fp64 sums, n x n, on the device -> `Distances`."""
        n = int(sums.shape[0]) if n is None else int(n)
        if _is_torch(sums) and (sums.dtype != _torch().float64 or not sums.is_contiguous() or not sums.is_cuda):
            raise ValueError('the sums must be a contiguous float64 CUDA tensor')
        with _Call(self, stream) as c:
            sums = c.as_it_lies(sums)
            dist = Distances(DeviceBuffer(self, (n, n), np.float32), n)
            c.run(self.lib.byz_manhattan_from_sums_dev(self.ctx, sums.ptr, n, dist.ptr, c.stream))
            self.synchronize(c.stream)
        return dist

    @staticmethod
    def _multi_metrics_keep(n, p=None, keep=None):
        """keep = int(p * n), checked as the library checks it (the refusals that need no GPU)."""
        n = int(n)
        if n > 16384:
            raise NotImplementedError('multi_metrics: at most 16384 rows, got %d' % n)
        if keep is None:
            p = float(p)
            if not p <= 1.0:
                raise ValueError('multi_metrics: p = %r must be at most 1' % p)
            keep = int(p * n)
            if keep < 1:
                raise ValueError('multi_metrics: int(p * n) = %d: p = %r keeps nobody of %d rows' % (keep, p, n))
        keep = int(keep)
        if keep < 1 or keep > n:
            raise ValueError('multi_metrics: keep = %d outside 1..%d (the row count)' % (keep, n))
        return keep

    def multi_metrics_info(self):
        """{kept, usable, degenerate, det} of the last multi_metrics_select or multi_metrics on this engine (synchronises): the
        rows chosen, the rows with three finite features, whether the degenerate rule (the Manhattan feature alone) scored
        them, and the determinant of the features' correlation matrix."""
        return dict(zip(('kept', 'usable', 'degenerate', 'det'),
                        self._read(self.lib.byz_multi_metrics_info, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_double])))

    def multi_metrics_features(self, man, euc, cos):
        """Multi-Metrics' features from three distance matrices (`Distances` handles or dense matrices with an infinite
        diagonal: Manhattan, Euclidean, cosine -- or any three): an (n, 3) float64 numpy array, row i = the sums of row i of
        each matrix over the usable j != i, (inf, inf, inf) for a row that is not usable (no finite off-diagonal cosine)."""
        if any(isinstance(d, dict) for d in (man, euc, cos)):
            raise ValueError('multi_metrics_features() takes Distances handles or dense matrices')
        with _Call(self) as c:
            ds = [c.distances(d)[0] for d in (man, euc, cos)]
            n = ds[0].n
            if any(d.n != n for d in ds):
                raise ValueError('the three distance matrices have %s rows' % ', '.join(str(d.n) for d in ds))
            self._multi_metrics_keep(n, keep=1)
            feat = DeviceBuffer(self, (n, 3), np.float64)
            c.run(self.lib.byz_multi_metrics_features_dev(self.ctx, ds[0].ptr, ds[1].ptr, ds[2].ptr, n, feat.ptr, None))
            return feat.numpy()

    def multi_metrics_select(self, features, keep, on_device=False, return_scores=False, like=None):
        """Multi-Metrics' scores and selection on an (n, 3) feature matrix (float64; multi_metrics_features' or the caller's
        own): the squared Mahalanobis norm of x / s under the features' correlation matrix, uncentred, and the min(usable,
        keep) rows of smallest (score, row) (include/byzagg.h).  Returns (rows, info) or (rows, scores, info): the chosen
        rows ascending (on_device=True: the 0 / 1 int32 flags instead, as a DeviceBuffer, or a torch tensor beside `like`),
        the float64 scores (+inf for a row that is not usable) and {kept, usable, degenerate, det}."""
        with _Call(self) as c:
            host = None if _is_device(features) else np.ascontiguousarray(_to_host(features), dtype=np.float64)
            shape = tuple(features.shape) if host is None else host.shape
            if len(shape) != 2 or shape[1] != 3:
                raise ValueError('multi_metrics_select: the features must be (n, 3), got %r' % (shape,))
            n = int(shape[0])
            keep = self._multi_metrics_keep(n, keep=keep)
            f = c.operand(features if host is None else host.reshape(-1), np.float64, _F64, 3 * n)
            if on_device and like is not None:
                c.beside(like, on_its_stream=False)
            flags, fptr = c.out(n, np.int32)
            scores, sptr = c.out(n, np.float64, want=return_scores)
            c.run(self.lib.byz_multi_metrics_select_dev(self.ctx, f.ptr, n, keep, fptr, sptr, None))
            info = self.multi_metrics_info()
            rows = flags if on_device else np.flatnonzero(_to_host(flags) if _is_torch(flags) else flags.numpy()).astype(np.int64)
            if return_scores:
                scores = _to_host(scores) if _is_torch(scores) else scores.numpy()
        return (rows, scores, info) if return_scores else (rows, info)

    def multi_metrics(self, g, p=0.3, return_info=False):
        """Multi-Metrics in one library call: the Manhattan, Euclidean and cosine matrices (one Gram for the last two), the
        features over the usable rows (Gram diagonal finite and > 0), multi_metrics_select with keep = int(p * n), and
        np.mean(g[chosen], axis=0) bit for bit.  Nobody usable: the zero vector.  return_info=True also returns {chosen_rows
        (ascending), kept, usable, degenerate, det}."""
        dm = self._device_matrix(g)
        n = dm.rows if dm is not None else self._host_matrix(g).shape[0]
        keep = self._multi_metrics_keep(n, p=p)
        with _Call(self) as c:
            if dm is None:
                h = self._host_matrix(g)
                d = h.shape[1]
                out = np.empty(d, dtype=np.float32)
                flags = np.zeros(n, dtype=np.int32)
                _check(self.lib.byz_multi_metrics_host(self.ctx, _hp(h), n, d, keep, _hp(out), _hp(flags)))
            else:
                dm = c.matrix(dm)
                out, optr = c.out(dm.cols)
                flags, fptr = c.out(n, np.int32, want=return_info)
                c.run(self.lib.byz_multi_metrics_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, keep, optr, fptr, c.stream))
                self.check(c.stream)      # (a kernel of the Gram can only flag a failure)
                if return_info:
                    flags = _to_host(flags) if _is_torch(flags) else flags.numpy()
        if not return_info:
            return out
        info = self.multi_metrics_info()
        info['chosen_rows'] = np.flatnonzero(flags).astype(np.int64)
        return out, info

    # ---- DnC, the spectral defence (Shejwalkar & Houmansadr 2021, Algorithm 2; not in the reference) ----
    def _dnc_lists(self, columns, n_cols, validate=True):
        """columns -> an (n_iters, b) int64 array of column lists: a torch CUDA tensor where it was one, else numpy.  One list
        (1-D) or one per iteration (2-D).  DnC's own contract is checked here unless the caller vouches: every list in range
        and strictly ascending (for a torch CUDA tensor one reduction and a host synchronisation)."""
        if _is_torch(columns) and columns.is_cuda:
            t = columns.reshape(1, -1) if columns.dim() == 1 else columns
            if t.dim() != 2 or t.dtype != _torch().int64 or t.device.index != self.device or t.numel() == 0:
                raise ValueError('device column lists must be a non-empty 1-D or 2-D int64 tensor on cuda:%d' % self.device)
            t = t.contiguous()
            bad = validate and (bool(((t < 0) | (t >= n_cols)).any().item()) or bool((t[:, 1:] <= t[:, :-1]).any().item()))
        else:
            t = _to_host(columns)
            if t.dtype.kind not in 'iu' or t.ndim not in (1, 2) or t.size == 0:
                raise ValueError('column lists must be a non-empty 1-D or 2-D integer array')
            t = np.ascontiguousarray(t.reshape(1, -1) if t.ndim == 1 else t, dtype=np.int64)
            bad = validate and (t.min() < 0 or t.max() >= n_cols or (np.diff(t, axis=1) <= 0).any())
        if bad:
            raise ValueError('column lists must be in [0, %d) and strictly ascending' % n_cols)
        return t

    def _dnc_operand(self, c, columns, n_cols, validate):
        return c.operand(self._dnc_lists(columns, n_cols, validate), np.int64, {}, (None, None), convert=False)

    def dnc_info(self):
        """(kept_rows, inactive_rows) of the last DnC call on this engine (synchronises)."""
        return tuple(self._read(self.lib.byz_dnc_info, [ctypes.c_int64, ctypes.c_int64]))

    def dnc_scores(self, g, columns, power_iters=32, validate_columns=True):
        """One DnC iteration's scores for one list of sampled columns: the squared projection of every centred row on the
        top right singular vector of the sampled, centred matrix (power iteration from the row of largest norm), +inf for a
        row with a non-finite sampled value.  fp64: a torch tensor for a torch input, numpy for a host input."""
        with _Call(self) as c:
            m = c.matrix(g)
            cols = self._dnc_operand(c, columns, m.cols, validate_columns)
            if cols.rows != 1:
                raise ValueError('dnc_scores() takes one list of columns')
            out, optr = c.out(m.rows, np.float64)
            c.run(self.lib.byz_dnc_scores_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, cols.ptr, cols.cols, int(power_iters), optr,
                                              c.stream))
            return c.result(out)

    def _dnc_kept(self, good):
        """The rows DnC kept, read back: numpy unless they are a torch tensor."""
        kept, _ = self.dnc_info()
        return good.numpy()[:kept] if isinstance(good, DeviceBuffer) else good[:kept]

    def dnc_select(self, g, remove_count, columns, power_iters=32, validate_columns=True):
        """The rows DnC keeps, ascending: every iteration (one per list of `columns`) ranks the rows by (score, index) and
        removes the `remove_count` highest; the kept sets are intersected.  int32: a torch tensor for a torch input, numpy
        otherwise.  Synchronises (the count is read back)."""
        with _Call(self) as c:
            m = c.matrix(g)
            cols = self._dnc_operand(c, columns, m.cols, validate_columns)
            params = _native.DncParams(cols.rows, cols.cols, int(power_iters), int(remove_count))
            good, gptr = c.out(m.rows, np.int32)
            c.run(self.lib.byz_dnc_select_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, ctypes.byref(params), cols.ptr, gptr, None,
                                              c.stream))
            return self._dnc_kept(good)

    def dnc(self, g, remove_count, columns, power_iters=32, return_selection=False, validate_columns=True):
        """DnC: np.mean(g[good], axis=0) over the rows every iteration kept (`dnc_select`'s).  `columns`: one ascending list
        of distinct column indices per iteration (`dnc_columns` draws them).  No row kept: NaN.  Device input: nothing
        synchronises unless the selection is asked for."""
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            cols = _to_host(self._dnc_lists(columns, d, validate_columns))
            params = _native.DncParams(cols.shape[0], cols.shape[1], int(power_iters), int(remove_count))
            out = np.empty(d, dtype=np.float32)
            good = np.empty(n, dtype=np.int32)
            kept = ctypes.c_int64(0)
            _check(self.lib.byz_dnc_host(self.ctx, _hp(h), n, d, ctypes.byref(params), _hp(cols), _hp(out), _hp(good),
                                         ctypes.byref(kept)))
            return (out, good[:kept.value]) if return_selection else out
        with _Call(self) as c:
            dm = c.matrix(dm)
            cols = self._dnc_operand(c, columns, dm.cols, validate_columns)
            params = _native.DncParams(cols.rows, cols.cols, int(power_iters), int(remove_count))
            out, optr = c.out(dm.cols)
            good, gptr = c.out(dm.rows, np.int32, want=return_selection)
            c.run(self.lib.byz_dnc_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params), cols.ptr, optr, gptr,
                                       c.stream))
            return (out, self._dnc_kept(good)) if return_selection else out

    def dnc_sharded(self, g_local, remove_count, local_columns, sub_dim, power_iters=32, all_reduce=None,
                    return_selection=False):
        """The columns layout's DnC on this rank's slice (byz_dnc_sharded_dev): local_columns is one ascending list per
        iteration of the sampled columns this rank owns, as indices into its slice (a list may be empty); sub_dim the global
        sample size; all_reduce(tensor) sums a CUDA fp64 tensor in place over the ranks on the current stream (None: one
        rank).  Returns this rank's columns of the mean (and the kept rows, the same on every rank)."""
        with _Call(self) as c:
            dm = c.matrix(g_local, needs='dnc_sharded')
            lists = [np.ascontiguousarray(np.asarray(cl, dtype=np.int64).reshape(-1)) for cl in local_columns]
            for cl in lists:
                if cl.size and (cl.min() < 0 or cl.max() >= dm.cols or (np.diff(cl) <= 0).any()):
                    raise ValueError('local column lists must be in [0, %d) and strictly ascending' % dm.cols)
            counts = (ctypes.c_int64 * len(lists))(*[int(cl.size) for cl in lists])
            flat = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
            fptr = c.upload(flat).ptr if flat.size else None
            callback = self._allreduce_callback(all_reduce)
            params = _native.DncParams(len(lists), int(sub_dim), int(power_iters), int(remove_count))
            out, optr = c.out(dm.cols)
            good, gptr = c.out(dm.rows, np.int32, want=return_selection)
            c.run(self.lib.byz_dnc_sharded_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, ctypes.byref(params), fptr, counts,
                                               ctypes.cast(callback, ctypes.c_void_p), None, optr, gptr, c.stream))
            return (out, self._dnc_kept(good)) if return_selection else out

    # ---- malicious.py ------------------------------------------------------------------------
    def drift_attack(self, rows, num_std, write_back=False):
        """(drift, mean, std) over the rows; device inputs may be overwritten in place (write_back)."""
        dm = self._device_matrix(rows)
        if dm is None:
            g = self._host_matrix(rows)
            n, d = g.shape
            drift, mean, std = (np.empty(d, dtype=np.float32) for _ in range(3))
            _check(self.lib.byz_drift_attack_host(self.ctx, _hp(g), n, d, float(num_std), _hp(drift), _hp(mean), _hp(std)))
            return drift, mean, std
        with _Call(self) as c:
            m = c.matrix(dm)
            (drift, dptr), (mean, mptr), (std, sptr) = (c.out(m.cols) for _ in range(3))
            c.run(self.lib.byz_drift_attack_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, float(num_std), dptr, mptr, sptr,
                                                int(bool(write_back)), c.stream))
        return drift, mean, std

    # ---- the attacks of Fang et al. (USENIX Security 2020; not in the reference) ----
    def column_extremes(self, g, n_malicious):
        """(mean, lo, hi) per column in ONE read of g: no_defense's mean over ALL rows, np.fmin.reduce and np.fmax.reduce over
        the benign rows g[n_malicious:] (a NaN is skipped; no benign number: NaN).  numpy for a host matrix, else device
        vectors beside g."""
        with _Call(self) as c:
            m = c.matrix(g)
            (mean, mptr), (lo, lptr), (hi, hptr) = (c.out(m.cols) for _ in range(3))
            c.run(self.lib.byz_column_extremes_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(n_malicious), mptr, lptr, hptr,
                                                   c.stream))
            return c.result((mean, lo, hi))

    @staticmethod
    def _fang_params(b, partial, seed, round, column_offset, k_lo=3.0, k_hi=4.0):
        """byz_fang_params; b finite and > 1, 0 <= k_lo <= k_hi finite, 0 <= round < 2^32, column_offset >= 0; the seed is
        taken modulo 2^64."""
        b, k_lo, k_hi = float(b), float(k_lo), float(k_hi)
        if not partial and not (np.isfinite(b) and b > 1.0):
            raise ValueError('b = %r must be finite and > 1' % (b,))
        if partial and not (0.0 <= k_lo <= k_hi and np.isfinite(k_hi)):
            raise ValueError('0 <= k_lo <= k_hi, both finite, violated: %r, %r' % (k_lo, k_hi))
        if not 0 <= int(round) < (1 << 32):
            raise ValueError('round = %r must lie in [0, 2^32): the attacker row takes the counter\'s top word' % (round,))
        if int(column_offset) < 0:
            raise ValueError('column_offset = %r must be >= 0' % (column_offset,))
        return _native.FangParams(b, k_lo, k_hi, 1 if partial else 0, int(seed) & ((1 << 64) - 1), int(round), int(column_offset))

    def fang_trmean_attack(self, g, n_malicious, b=2.0, partial=False, seed=0, round=0, column_offset=0, k_lo=3.0, k_hi=4.0):
        """Fang et al.'s attack on the trimmed mean and the median (include/byzagg.h, rules A and B).  Rows 0 .. n_malicious - 1
        of g hold the attackers' honest gradients, the others are benign.  Full knowledge: per column the mean of all rows
        decides the side, every attacker value is drawn beyond the benign extreme of that side, from [lo / b, lo] or [b lo, lo]
        (mean > 0), [hi, b hi] or [hi, hi / b] (otherwise). partial=True: from the attacker rows' own mean and std, [mu - k_hi
        sigma, mu - k_lo sigma] or [mu + k_lo sigma, mu + k_hi sigma].  The draws come from the Philox stream of (seed, round,
        attacker row, global column): every attacker row its own numbers, a column slice with its column_offset the whole
        matrix's.  A device-resident g is attacked IN PLACE and its first n_malicious rows are returned as a view (torch) or
        None (DeviceBuffer); a host matrix is left alone and the attacked rows come back as numpy.  Nothing synchronises."""
        params = self._fang_params(b, partial, seed, round, column_offset, k_lo, k_hi)
        c_rows = int(n_malicious)
        dm = self._device_matrix(g)
        if dm is None:
            h = self._host_matrix(g)
            n, d = h.shape
            if not 0 <= c_rows <= n:
                raise ValueError('%d attacker rows of %d rows' % (c_rows, n))
            rows = np.empty((c_rows, d), dtype=np.float32)
            _check(self.lib.byz_fang_trmean_attack_host(self.ctx, _hp(h), n, d, c_rows, ctypes.byref(params), _hp(rows)))
            return rows
        with _Call(self) as c:
            dm = c.matrix(dm)
            c.run(self.lib.byz_fang_trmean_attack_dev(self.ctx, dm.ptr, dm.rows, dm.cols, dm.ld, c_rows, ctypes.byref(params),
                                                      c.stream))
        return g[:c_rows] if dm.torch_like is not None else None

    def fang_krum_info(self):
        """{lambda0, lambda, steps, chosen, succeeded} of the last fang_krum_attack on this engine (synchronises)."""
        lambda0, lam, steps, chosen, succeeded = self._read(
            self.lib.byz_fang_krum_info, [ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32])
        return {'lambda0': lambda0, 'lambda': lam, 'steps': steps, 'chosen': chosen, 'succeeded': bool(succeeded)}

    def fang_krum_attack(self, g, n_malicious, threshold=1e-5, return_info=False, return_working=False):
        """Fang et al.'s attack on Krum (include/byzagg.h, rule C): every attacker row becomes -lambda s, s the sign of the
        column means, lambda halved from Theorem 1's bound until the library's own Krum picks an attacker row or lambda falls
        below `threshold`.  The benign rows' distances are computed once; a step rewrites the attackers' rows and columns of
        the distance matrix from t = g . s and q = |g|^2 and runs krum_select: the host reads one index per step.  A
        device-resident g is attacked IN PLACE (returns its first rows as a view, or None for a DeviceBuffer); a host matrix is
        left alone and the attacked rows come back as numpy.  return_info=True adds fang_krum_info(); return_working=True adds
        to that dict the last step's `distances` (a Distances handle) and the benign rows' `t` and `q` (fp64)."""
        c_rows = int(n_malicious)
        threshold = ctypes.c_double(float(threshold))
        with _Call(self) as c:
            m = c.matrix(g)
            dist = DeviceBuffer(self, (m.rows, m.rows), np.float32) if return_working else None
            dptr = dist.ptr if return_working else None
            t, tptr = c.out(max(m.rows - c_rows, 1), np.float64, want=return_working)
            q, qptr = c.out(max(m.rows - c_rows, 1), np.float64, want=return_working)
            c.run(self.lib.byz_fang_krum_attack_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, c_rows, ctypes.byref(threshold), dptr,
                                                    tptr, qptr, c.stream))
            if c.host:
                rows = c.numpy(m.keep)[:c_rows]
            else:
                rows = g[:c_rows] if m.torch_like is not None else None
            if not (return_info or return_working):
                return rows
            info = self.fang_krum_info()
            if return_working:
                info['distances'] = Distances(dist, m.rows)
                info['t'], info['q'] = c.result((t, q))
            return rows, info

    # ---- the Min-Max / Min-Sum attacks of Shejwalkar & Houmansadr (NDSS 2021; not in the reference) ----
    def row_moments(self, g, z, p):
        """(a, b): a[i] = sum_c ((double)g[i, c] - (double)z[c])^2 (row_sqdist's bits) and b[i] = sum_c (double)p[c] *
        ((double)z[c] - (double)g[i, c]), both fp64 in a fixed order, in ONE read of g: |z + gamma p - g_i|^2 = a_i + 2 gamma b_i
        + gamma^2 |p|^2.  On one rank of the columns layout, its part over its columns.  fp64 out: torch tensors for a torch
        input, numpy for a host input, DeviceBuffers otherwise."""
        with _Call(self) as c:
            m = c.matrix(g)
            z = c.operand(z, np.float32, _f32('z has %(got)d entries, the matrix %(n)d columns'), m.cols, convert=False)
            p = c.operand(p, np.float32, _f32('p has %(got)d entries, the matrix %(n)d columns'), m.cols, convert=False)
            a, aptr = c.out(m.rows, np.float64)
            b, bptr = c.out(m.rows, np.float64)
            c.run(self.lib.byz_row_moments_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, z.ptr, p.ptr, aptr, bptr, c.stream))
            return c.result((a, b))

    @staticmethod
    def _minmax_params(kind, perturbation, partial, p, dist_given=False):
        """byz_minmax_params; refuses an unknown kind or perturbation, and a custom perturbation without its vector (or a vector
        without it), before anything is launched."""
        if kind not in MINMAX_KINDS:
            raise ValueError('kind = %r: one of %s' % (kind, sorted(MINMAX_KINDS)))
        if perturbation not in MINMAX_PERTURBATIONS:
            raise ValueError('perturbation = %r: one of %s' % (perturbation, sorted(MINMAX_PERTURBATIONS)))
        if (perturbation == 'custom') != (p is not None):
            raise ValueError("perturbation='custom' and the vector p come together or not at all")
        return _native.MinmaxParams(MINMAX_KINDS[kind], MINMAX_PERTURBATIONS[perturbation], 1 if partial else 0, 1 if dist_given else 0)

    def minmax_info(self):
        """{gamma, bound, c, binding_row, known_rows, degenerate, broken} of the last minmax_attack on this engine
        (synchronises).  bound: T = Dmax^2 for Min-Max, S = r max a_i + A for Min-Sum."""
        gamma, bound, c, row, r, degenerate, broken = self._read(
            self.lib.byz_minmax_info, [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_int32, ctypes.c_int32])
        return {'gamma': gamma, 'bound': bound, 'c': c, 'binding_row': row, 'known_rows': r, 'degenerate': bool(degenerate),
                'broken': bool(broken)}

    def minmax_attack(self, g, n_malicious, kind='minmax', perturbation='std', partial=False, p=None, return_info=False,
                      distances=None, all_reduce=None):
        """The Min-Max (kind='minmax') and Min-Sum ('minsum') attacks (include/byzagg.h, rule D).  Rows 0 .. n_malicious - 1 of
        g hold the attackers' honest gradients; the known rows are all of them, or with partial=True the attackers' own.  Every
        attacker row becomes the ONE vector mu + gamma p: mu the known rows' mean, p the perturbation ('unit': -mu / |mu|,
        'std': -std, the population estimate, 'sign': -sign(mu), 'custom': the vector `p`), gamma the largest that keeps the
        vector as close to every known row as they are to each other -- in closed form, no search.  A device-resident g is
        attacked IN PLACE and its first n_malicious rows are returned as a view (torch) or None (DeviceBuffer); a host matrix
        is left alone and the ONE attacked vector comes back as numpy.  distances: a Distances handle of ALL rows for Min-Max
        (skips the Gram).  all_reduce: g is this rank's column slice (columns layout; a device matrix).  return_info=True adds
        minmax_info().  A broken input (a value that is not finite among the known rows) leaves the rows as they were."""
        params = self._minmax_params(kind, perturbation, partial, p, dist_given=distances is not None)
        c_rows = int(n_malicious)
        dm = self._device_matrix(g)
        if dm is None and all_reduce is None and distances is None:
            h = self._host_matrix(g)
            n, d = h.shape
            if not 1 <= c_rows <= n:
                raise ValueError('%d attacker rows of %d rows' % (c_rows, n))
            pv = None if p is None else np.ascontiguousarray(_to_host(p), dtype=np.float32).reshape(-1)
            if pv is not None and pv.size != d:
                raise ValueError('p has %d entries, the matrix %d columns' % (pv.size, d))
            vec = np.empty(d, dtype=np.float32)
            _check(self.lib.byz_minmax_attack_host(self.ctx, _hp(h), n, d, c_rows, ctypes.byref(params), _hp(pv), _hp(vec)))
            return (vec, self.minmax_info()) if return_info else vec
        with _Call(self) as c:
            m = c.matrix(g, needs='minmax_attack' if dm is None else None)
            pv = None
            if p is not None:
                pv = c.operand(p, np.float32, _f32('p has %(got)d entries, the matrix %(n)d columns'), m.cols, convert=False).ptr
            dptr = distances.ptr if distances is not None else None
            if distances is not None and distances.n != m.rows:
                raise ValueError('the distance matrix has %d rows, the gradient matrix %d' % (distances.n, m.rows))
            if all_reduce is None:
                c.run(self.lib.byz_minmax_attack_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, c_rows, ctypes.byref(params), pv, dptr,
                                                     c.stream))
            else:
                callback = self._allreduce_callback(all_reduce)
                c.run(self.lib.byz_minmax_attack_sharded_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, c_rows, ctypes.byref(params), pv,
                                                             dptr, ctypes.cast(callback, ctypes.c_void_p), None, c.stream))
            rows = g[:c_rows] if m.torch_like is not None else None
            return (rows, self.minmax_info()) if return_info else rows

    def column_chain(self, rows, carry=None, mean=None):
        """One link of the attack's statistics over rows that several owners hold (sharded.py, clients layout): the running
        column sums after THESE rows, continuing `carry` (the previous owner's result; None: the chain starts here) -- of the
        values, or with `mean` of their squared fp32 deviations.  Device tensors in, a device vector out."""
        m = self._device_matrix(rows)
        if m is None or m.torch_like is None:
            raise ValueError('column_chain() takes a torch CUDA matrix')
        for v in (carry, mean):
            if v is not None and (not _is_torch(v) or v.dtype != _torch().float32 or not v.is_contiguous() or v.numel() != m.cols
                                  or v.device != m.torch_like.device):
                raise ValueError('carry / mean must be contiguous float32 vectors of %d columns on the matrix\'s device' % m.cols)
        with _Call(self) as c:
            m = c.matrix(m)
            out, optr = c.out(m.cols)
            c.run(self.lib.byz_column_chain_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld,
                                                carry.data_ptr() if carry is not None else None,
                                                mean.data_ptr() if mean is not None else None, optr, c.stream))
        return out

    def column_finish(self, total_rows, num_std, sum=None, sumsq=None, mean=None):
        """The end of a chain.  sum given: returns mean = sum / total_rows.  sumsq (and mean) given: returns (std, drift) =
        (sqrt(sumsq / total_rows), mean - num_std * std)."""
        torch = _torch()
        if (sum is None) == (sumsq is None):
            raise ValueError('column_finish: give the sum (returns the mean) or the sum of squared deviations (returns std, drift)')
        if sum is None and mean is None:
            raise ValueError('column_finish: the squared deviations need the mean they were taken about')
        ref = sum if sum is not None else sumsq
        for name, t in (('sum', sum), ('sumsq', sumsq), ('mean', mean)):
            if t is None:
                continue
            if not (_is_torch(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError('column_finish: %s must be a contiguous float32 CUDA tensor' % name)
            if t.numel() != ref.numel() or t.device != ref.device:
                raise ValueError('column_finish: %s has %d values on %s, expected %d on %s' % (name, t.numel(), t.device, ref.numel(), ref.device))
        n = ref.numel()
        stream = _stream_of(ref)
        if sum is not None:
            mean = torch.empty_like(sum)
            _check(self.lib.byz_column_finish_dev(self.ctx, sum.data_ptr(), None, int(total_rows), float(num_std), n,
                                                  mean.data_ptr(), None, None, stream))
            return mean
        std, drift = torch.empty_like(sumsq), torch.empty_like(sumsq)
        _check(self.lib.byz_column_finish_dev(self.ctx, None, sumsq.data_ptr(), int(total_rows), float(num_std), n,
                                              mean.data_ptr(), std.data_ptr(), drift.data_ptr(), stream))
        return std, drift

    def drift_axpy_host(self, mean, std, num_std):
        """DriftAttack._attack_grads on host vectors (malicious.py:34-36), computed on the device."""
        mean_c = np.ascontiguousarray(mean, dtype=np.float32)
        a, b = self.to_device(mean_c), self.to_device(np.ascontiguousarray(std, dtype=np.float32))
        _check(self.lib.byz_drift_axpy_dev(self.ctx, a.ptr, b.ptr, mean_c.size, float(num_std), None))
        return a.numpy()

    # ---- server.py:89-90 ---------------------------------------------------------------------
    def server_update(self, weights, velocity, agg, momentum, learning_rate):
        """In-place fused momentum update on device-resident vectors (torch tensors or DeviceBuffers)."""
        with _Call(self) as c:
            w, v, a = c.as_it_lies(weights), c.as_it_lies(velocity), c.as_it_lies(agg)
            c.run(self.lib.byz_server_update_dev(self.ctx, w.ptr, v.ptr, a.ptr, w.size, float(momentum), float(learning_rate),
                                                 c.stream))

    # ---- backdoor.py:52-65 (the hook's arithmetic; the training loop stays with the caller) ----
    def _vector_rule(self, launch, *vectors):
        """A rule on same-length float32 vectors: host vectors are uploaded, torch CUDA tensors and DeviceBuffers used in place;
        numpy out when every vector came from the host, else device-resident."""
        with _Call(self) as c:
            ops = [c.operand(vectors[0], np.float32, _f32(None), convert=False, leads=True)]
            ops += [c.operand(v, np.float32, _DIFFER, ops[0].size, convert=False, leads=True) for v in vectors[1:]]
            out, optr = c.out(ops[0].size)
            c.run(launch([op.ptr for op in ops], ops[0].size, optr, c.stream))
            return c.result(out)

    def backdoor_initial_params(self, original_params, grads_mean, learning_rate):
        """original_params - learning_rate * grads_mean (backdoor.py:54).  numpy in -> numpy out;
        device-resident in -> device-resident out."""
        return self._vector_rule(lambda p, n, optr, stream: self.lib.byz_backdoor_initial_params_dev(
            self.ctx, p[0], p[1], n, float(np.float32(learning_rate)), optr, stream), original_params, grads_mean)

    def backdoor_clip(self, grads_mean, grads_stdev, original_params, mal_net_params, learning_rate, num_std):
        """The gradient that leads to `mal_net_params`, clipped to mean +- num_std * std (backdoor.py:57-63)."""
        return self._vector_rule(lambda p, n, optr, stream: self.lib.byz_backdoor_clip_dev(
            self.ctx, p[0], p[1], p[2], p[3], n, float(np.float32(learning_rate)), float(np.float32(num_std)), optr, stream),
            grads_mean, grads_stdev, original_params, mal_net_params)

    # ---- user.py:92 + server.py:81-83 --------------------------------------------------------------
    def assemble_row(self, g, row, grads):
        """Row `row` of the device-resident matrix `g` := the client's gradient.

        `grads` is either the client's flat vector (numpy, what `usr.grads` is in the reference: one
        host-to-device copy) or a sequence of device tensors, one per model parameter in parameter order
        (torch CUDA tensors or DeviceBuffers): those are concatenated straight into the row by one kernel,
        and the gradient never visits the host."""
        m = self._device_matrix(g)
        if m is None:
            raise ValueError('assemble_row() fills a device-resident matrix')
        if isinstance(grads, (list, tuple)):
            ptrs, lens, keep = self._segments(grads, None, 'gradient tensors must be float32',
                                              'a list of gradients must hold device tensors; pass host data as one flat vector')
            sync_after = self._order_after_torch(m, keep)
            table = (ctypes.c_void_p * len(ptrs))(*ptrs)
            lengths = (ctypes.c_int64 * len(lens))(*lens)
            _check(self.lib.byz_assemble_row_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(row), len(ptrs),
                                                 table, lengths, m.stream))
            if sync_after:
                self.synchronize(m.stream)
            return
        host = grads.detach().cpu().numpy() if _is_torch(grads) else np.asarray(grads)
        host = np.ascontiguousarray(host, dtype=np.float32).ravel()
        if host.size != m.cols:
            raise ValueError('the row holds %d values, the gradient %d' % (m.cols, host.size))
        _check(self.lib.byz_assemble_row_host(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(row),
                                              _hp(host), m.stream))
        self.synchronize(m.stream)   # `host` may be a temporary

    @staticmethod
    def _segments(tensors, rows, not_float32, not_device):
        """Device tensors (float32: torch CUDA tensors or DeviceBuffers) -> (pointers, lengths, keep-alives).  `rows`: None, or
        the leading dimension every tensor must have (the lengths are then per row).  A torch tensor that is not contiguous is
        replaced by a contiguous temporary: its keep-alive is then not the caller's tensor."""
        ptrs, lens, keep = [], [], []
        for t in tensors:
            if isinstance(t, DeviceBuffer):
                assert t.dtype == np.float32 and (rows is None or t.shape[0] == rows)
                ptr, size = t.ptr, int(np.prod(t.shape))
            elif _is_torch(t) and t.is_cuda:
                torch = _torch()
                if t.dtype != torch.float32 or (rows is not None and t.shape[0] != rows):
                    raise ValueError(not_float32)
                t = t if t.is_contiguous() else t.contiguous()
                ptr, size = t.data_ptr(), t.numel()
            else:
                raise ValueError(not_device)
            ptrs.append(ptr)
            lens.append(size // (rows or 1))
            keep.append(t)
        return ptrs, lens, keep

    def _order_after_torch(self, m, tensors):
        """The launch goes to m.stream; torch tensors (and the .contiguous() temporaries made of them) belong to torch's
        current stream.  Where the two differ -- a DeviceBuffer matrix filled from torch tensors under a side stream --
        the producers are waited for before the launch and the launch before the temporaries can be freed.
        Returns whether the caller must synchronise m.stream after the launch."""
        for t in tensors:
            if _is_torch(t):
                torch = _torch()
                current = torch.cuda.current_stream(t.device)
                if int(current.cuda_stream) != int(m.stream or 0):
                    current.synchronize()
                    return True
                return False
        return False

    def assemble_rows(self, g, first_row, clients_grads):
        """Rows first_row .. of the device-resident matrix := the clients' gradients, ONE launch for all of them
        (server.py:81-83's loop).  `clients_grads[c]` is client c's sequence of device tensors, one per model parameter in
        parameter order; every client has the same parameter sizes (one model).

        The table of the clients' tensor addresses is built and uploaded when an address changed since the last call; a round
        in which no tensor moved (the normal case: a model's .grad buffers keep their addresses) costs one pass over
        `data_ptr()` and the launch (the table of 400 tensors was rebuilt and uploaded every round, twelve
        times the kernel's own time)."""
        m = self._device_matrix(g)
        if m is None:
            raise ValueError('assemble_rows() fills a device-resident matrix')
        n_clients = len(clients_grads)
        if n_clients == 0:
            return
        n_seg = len(clients_grads[0])
        key = None
        if n_seg and _is_torch(clients_grads[0][0]):
            torch = _torch()
            try:     # C-level chain + map: no Python frame per tensor, no intermediate list
                first = clients_grads[0]
                # The table on the device is only valid for THESE tensors: the addresses of all of them, and -- because the
                # caching allocator can hand the same addresses back to tensors of another dtype or another split -- the
                # element counts, dtypes and contiguity of one client's tensors (every client has the same sizes: checked when
                # the table was built).  The fast path also skips the stream ordering of the general path, so it is only
                # taken when the launch stream IS torch's current stream.
                key = (n_clients, n_seg, m.cols, int(m.stream or 0),
                       int(torch.cuda.current_stream(first[0].device).cuda_stream),
                       tuple((t.numel(), t.dtype, t.is_contiguous()) for t in first),
                       tuple(map(torch.Tensor.data_ptr, itertools.chain.from_iterable(clients_grads))))
                if key[3] != key[4]:
                    key = None
            except (TypeError, AttributeError):
                key = None      # DeviceBuffers among them: the general path below
        if key is not None and key == self._assemble_key:      # (equal keys: equal tensor counts too)
            _check(self.lib.byz_assemble_rows_again_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(first_row), n_clients,
                                                        n_seg, m.stream))
            return
        self._assemble_key = None
        flat = list(itertools.chain.from_iterable(clients_grads))
        if len(flat) != n_clients * n_seg:
            raise ValueError('every client must hand over the same number of tensors')
        ptrs, keep, lens = [], [], None
        for c in range(n_clients):
            p, mine, k = self._segments(flat[c * n_seg:(c + 1) * n_seg], None, 'gradient tensors must be float32',
                                        'assemble_rows() takes device tensors; host vectors go through assemble_row()')
            ptrs += p
            keep += k
            if lens is None:
                lens = mine
            elif mine != lens:
                raise ValueError('clients disagree on the parameter sizes: %r and %r' % (lens, mine))
        sync_after = self._order_after_torch(m, keep)
        table = (ctypes.c_void_p * len(ptrs))(*ptrs)
        lengths = (ctypes.c_int64 * n_seg)(*lens)
        _check(self.lib.byz_assemble_rows_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, int(first_row), n_clients, n_seg,
                                              table, lengths, m.stream))
        if sync_after:
            self.synchronize(m.stream)
        if key is not None and all(k is t for k, t in zip(keep, flat)):      # (no contiguous temporaries among them)
            self._assemble_key = key      # what the device table now holds

    def assemble_columns(self, g, batched_grads):
        """Every client at once: `batched_grads[s]` is the device tensor (n_clients, *shape_s) holding parameter
        s's gradient for all clients (a batched client step); `g[:, start_s:start_s + len_s]` := its rows."""
        m = self._device_matrix(g)
        if m is None:
            raise ValueError('assemble_columns() fills a device-resident matrix')
        ptrs, lens, keep = self._segments(batched_grads, m.rows, 'batched gradients must be float32 with one leading row per client',
                                          'batched gradients must be device tensors')
        sync_after = self._order_after_torch(m, keep)
        table = (ctypes.c_void_p * len(ptrs))(*ptrs)
        lengths = (ctypes.c_int64 * len(lens))(*lens)
        _check(self.lib.byz_assemble_columns_dev(self.ctx, m.ptr, m.rows, m.cols, m.ld, len(ptrs), table, lengths,
                                                 m.stream))
        if sync_after:
            self.synchronize(m.stream)

    # ---- timing ------------------------------------------------------------------------------
    def timing(self, on=True):
        _check(self.lib.byz_timing_enable(self.ctx, int(bool(on))))
        _check(self.lib.byz_timing_reset(self.ctx))

    def timing_read(self):
        out = {}
        for k, name in enumerate(_native.KERNELS):
            ms, calls = ctypes.c_double(0.0), ctypes.c_int64(0)
            _check(self.lib.byz_timing_read(self.ctx, k, ctypes.byref(ms), ctypes.byref(calls)))
            if calls.value:
                out[name] = {'total_ms': ms.value, 'launches': calls.value}
        return out

    def lane_exchange_selftest(self, reductions=False):
        """The self-test kernel's rows of 64 lanes: the 11 lane_xor patterns, or with `reductions` the rows behind them
        (every lane's result of one of lane_exchange.hpp's wave reductions each)."""
        buf = DeviceBuffer(self, (64 * 64,), np.int32)
        n = ctypes.c_int32(0)
        _check(self.lib.byz_selftest_lane_exchange_dev(self.ctx, buf.ptr, ctypes.byref(n), None))
        self.synchronize()
        rows = buf.numpy()[: n.value * 64].reshape(n.value, 64)
        return rows[11:] if reductions else rows[:11]

    def owner_loop_selftest(self):
        """The rows of 1024 words that owner_loop.hpp's self-test kernel writes, one word a thread of its one workgroup."""
        buf = DeviceBuffer(self, (64 * 1024,), np.int32)
        n = ctypes.c_int32(0)
        _check(self.lib.byz_selftest_owner_loop_dev(self.ctx, buf.ptr, ctypes.byref(n), None))
        self.synchronize()
        return buf.numpy()[: n.value * 1024].reshape(n.value, 1024)


_default = None


def get_engine():
    """Process-wide engine on BYZ_DEVICE / LOCAL_RANK (default GPU 0); created on first use."""
    global _default
    if _default is None:
        _default = Engine()
    return _default
