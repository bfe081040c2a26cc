"""``DeviceTable``: one replica's row table on one MI355X, over the C-ABI.

Columns may be numpy arrays (host memory, staged by the library) or torch
tensors already resident on the GPU (zero-copy: their device pointers are
passed straight through, ``CRDT_MEM_DEVICE``).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi
from ._capi import CrdtBatch, CrdtResult, CrdtTiming


class CrdtNativeError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = _capi.status_string(status) if status else "ok"
        super().__init__(f"{what}: {msg} ({status})" if what else f"{msg} ({status})")


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


_NP_TYPES = {"u4": np.uint32, "i8": np.int64, "u1": np.uint8}
# torch dtypes a device column of each kind may have (same element width; the kernels
# reinterpret the bits, so int32 carries uint32 ids / handles)
_TORCH_KINDS = {"u4": ("int32", "uint32"), "i8": ("int64",), "u1": ("uint8", "bool")}


def check_device_tensor(t, kind: str, device: int, name: str = "tensor"):
    """A GPU tensor handed to the library by pointer: contiguous, of the kind's element width
    and on the ctx's device (the kernels index it by element; a wrong width reads past its end)."""
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    dt = str(t.dtype).replace("torch.", "")
    if dt not in _TORCH_KINDS[kind]:
        raise ValueError(f"{name}: dtype {dt} where {'/'.join(_TORCH_KINDS[kind])} is expected")
    if t.device.index is not None and device is not None and t.device.index != device:
        raise ValueError(f"{name} is on cuda:{t.device.index}, the table on cuda:{device}")


def torch_ready(t):
    """The library reads device columns on its own HIP stream, but torch produced them on torch's
    current stream (asynchronously): that stream's pending work on the tensor's device is finished
    before the pointer is handed over (the C-ABI's contract: resident columns are ready when a crdt_*
    call starts; the call itself returns only when its stream is done, so outputs need nothing)."""
    import torch
    torch.cuda.current_stream(t.device).synchronize()


class _Cols:
    """Normalises a set of columns to one memory kind and keeps them alive."""

    def __init__(self, device=None, **cols):
        self.keep = []
        self.mem = None
        self.ptrs = {}
        for name, (arr, kind) in cols.items():
            if arr is None:
                self.ptrs[name] = None
                continue
            if _is_torch(arr):
                if not arr.is_cuda:
                    arr = arr.numpy()
                else:
                    check_device_tensor(arr, kind, device, f"column {name}")
                    if not self.keep or not _is_torch(self.keep[0]):
                        torch_ready(arr)
                    mem = _capi.CRDT_MEM_DEVICE
                    self._set_mem(mem)
                    self.keep.append(arr)
                    self.ptrs[name] = ctypes.c_void_p(arr.data_ptr())
                    continue
            a = np.ascontiguousarray(arr, dtype=_NP_TYPES[kind])
            self._set_mem(_capi.CRDT_MEM_HOST)
            self.keep.append(a)
            self.ptrs[name] = a.ctypes.data_as(ctypes.c_void_p)
        if self.mem is None:
            self.mem = _capi.CRDT_MEM_HOST

    def _set_mem(self, mem):
        if self.mem is None:
            self.mem = mem
        elif self.mem != mem:
            raise ValueError("all columns of one call must live in the same memory (host or device)")


class Export:
    """A device-resident changeset (``crdt_export``): ``n`` records, ``n_live`` of them not
    tombstones.  It belongs to the table that exported it and ends at that table's next
    ``export_since``, ``export_flagged``, ``export_release`` or ``close``; a view that has ended raises
    ``CrdtNativeError(CRDT_E_INVALID)`` (the state is checked on the host, no memory is read)."""

    def __init__(self, table: "DeviceTable", view, serial: int):
        self._table = table
        self._view = view
        self._serial = serial
        self.n = int(view.n)
        self.n_live = int(view.n_live)
        self.device = int(view.device)

    def columns(self, first: int = 0, count: int | None = None):
        """Host copies ``key, lt, rank, val, mod`` of records [first, first + count)."""
        t = self._table
        if self._serial != getattr(t, "_export_serial", 0) or not (t._ctx and t._ctx.value):
            raise CrdtNativeError(_capi.CRDT_E_INVALID, "crdt_export_read (the view was replaced)")
        count = self.n - first if count is None else int(count)
        if first < 0 or count < 0:
            raise CrdtNativeError(_capi.CRDT_E_INVALID, "crdt_export_read")
        m = max(count, 0)
        key, rank, val = np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(m, np.uint32)
        lt, mod = np.empty(m, np.int64), np.empty(m, np.int64)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        t._check(t._lib.crdt_export_read(t._ctx, int(first), count, P(key), P(lt), P(rank), P(val), P(mod)),
                 "crdt_export_read")
        return key, lt, rank, val, mod


class DeviceTable:
    """Rows ``{lt, rank, val, mod}`` indexed by key id, plus the canonical clock."""

    def __init__(self, device: int = 0, local_rank: int = 0, capacity: int = 1024):
        self._lib = _capi.load()
        self._ctx = ctypes.c_void_p()
        st = self._lib.crdt_create(device, local_rank, max(int(capacity), 16), ctypes.byref(self._ctx))
        if st != 0:
            raise CrdtNativeError(st, "crdt_create")
        self.device = device
        self._local_rank = local_rank

    # ---------------------------------------------------------------- lifecycle
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.crdt_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dptr(self, t, kind: str, name: str):
        """Device pointer of a GPU tensor argument after the width / device checks."""
        check_device_tensor(t, kind, self.device, name)
        torch_ready(t)
        return ctypes.c_void_p(t.data_ptr())

    def _check(self, st: int, what: str):
        if st < 0:
            raise CrdtNativeError(st, what)
        return st

    @property
    def capacity(self) -> int:
        v = ctypes.c_uint64()
        self._check(self._lib.crdt_capacity(self._ctx, ctypes.byref(v)), "crdt_capacity")
        return v.value

    def reserve(self, capacity: int):
        if capacity > self.capacity:
            cap = max(int(capacity), 2 * self.capacity)
            self._check(self._lib.crdt_reserve(self._ctx, cap), "crdt_reserve")

    @property
    def canonical(self) -> int:
        v = ctypes.c_int64()
        self._check(self._lib.crdt_get_canonical(self._ctx, ctypes.byref(v)), "crdt_get_canonical")
        return v.value

    @canonical.setter
    def canonical(self, lt: int):
        self._check(self._lib.crdt_set_canonical(self._ctx, int(lt)), "crdt_set_canonical")

    @property
    def local_rank(self) -> int:
        return self._local_rank

    @local_rank.setter
    def local_rank(self, r: int):
        self._check(self._lib.crdt_set_local_rank(self._ctx, int(r)), "crdt_set_local_rank")
        self._local_rank = int(r)

    # ---------------------------------------------------------------------- SPI
    def put_rows(self, key, lt, rank, val, mod):
        c = _Cols(self.device, key=(key, "u4"), lt=(lt, "i8"), rank=(rank, "u4"), val=(val, "u4"), mod=(mod, "i8"))
        n = len(key)
        p = c.ptrs
        self._check(self._lib.crdt_put_rows(self._ctx, p["key"], p["lt"], p["rank"], p["val"], p["mod"],
                                            n, c.mem), "crdt_put_rows")

    def read_rows(self, key):
        key = np.ascontiguousarray(key, dtype=np.uint32)
        n = len(key)
        lt = np.empty(n, np.int64)
        rank = np.empty(n, np.uint32)
        val = np.empty(n, np.uint32)
        mod = np.empty(n, np.int64)
        if n:
            P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            self._check(self._lib.crdt_read_rows(self._ctx, P(key), n, P(lt), P(rank), P(val), P(mod),
                                                 _capi.CRDT_MEM_HOST), "crdt_read_rows")
        return lt, rank, val, mod

    def modified_since(self, n_rows: int, since: int) -> np.ndarray:
        out = np.empty(max(n_rows, 1), np.uint32)
        n = ctypes.c_uint64()
        self._check(self._lib.crdt_modified_since(self._ctx, n_rows, int(since),
                                                  out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)),
                    "crdt_modified_since")
        return out[:n.value]

    # ------------------------------------- changeset export (crdt_export_since)
    def export_since(self, n_rows: int, since: int) -> "Export":
        """recordMap(modifiedSince) left on the device: the rows of [0, n_rows) with mod >= since as
        one changeset, ascending by id.  The view ends at this table's next export_since / release."""
        v = _capi.CrdtExport()
        self._check(self._lib.crdt_export_since(self._ctx, int(n_rows), int(since), ctypes.byref(v)),
                    "crdt_export_since")
        self._export_serial = getattr(self, "_export_serial", 0) + 1
        return Export(self, v, self._export_serial)

    def export_flagged(self, n_rows: int, flags, bits: int = 0xFF) -> "Export":
        """The rows of [0, n_rows) whose ``flags[i] & bits`` is non-zero as one changeset, ascending by id
        (``crdt_export_flagged``): the winners of a table merge, read from the table they came from with the
        merge's row flags or mask.  ``flags``: a torch uint8/bool CUDA tensor of at least ``n_rows`` entries.
        The view replaces this table's earlier one, as ``export_since``'s does."""
        n_rows, bits = int(n_rows), int(bits)
        if not 0 <= bits <= 0xFF:
            raise ValueError(f"export_flagged: bits {bits:#x} is not a byte")
        mem = _capi.CRDT_MEM_DEVICE
        if _is_torch(flags) and flags.is_cuda:
            if flags.numel() < n_rows:
                raise ValueError("export_flagged: flags must hold one entry per row")
            fptr = self._dptr(flags, "u1", "flags")
        else:                                           # host memory: the library refuses it (CRDT_E_INVALID)
            flags = np.ascontiguousarray(flags.numpy() if _is_torch(flags) else flags, dtype=np.uint8)
            if len(flags) < n_rows:
                raise ValueError("export_flagged: flags must hold one entry per row")
            fptr, mem = flags.ctypes.data_as(ctypes.c_void_p), _capi.CRDT_MEM_HOST
        v = _capi.CrdtExport()
        self._check(self._lib.crdt_export_flagged(self._ctx, n_rows, fptr, mem, bits, ctypes.byref(v)),
                    "crdt_export_flagged")
        self._export_serial = getattr(self, "_export_serial", 0) + 1
        return Export(self, v, self._export_serial)

    def export_live(self, n_rows: int) -> "Export":
        """The ``map`` getter's rows (``crdt_export_live``): the records of ``export_since(n_rows, 0)`` that
        are not tombstones, in the same order, so ``n == n_live``.  The view replaces this table's earlier
        one, as ``export_since``'s does."""
        v = _capi.CrdtExport()
        self._check(self._lib.crdt_export_live(self._ctx, int(n_rows), ctypes.byref(v)), "crdt_export_live")
        self._export_serial = getattr(self, "_export_serial", 0) + 1
        return Export(self, v, self._export_serial)

    def count_since(self, n_rows: int, since: int) -> tuple[int, int]:
        """(records, live records) export_since would select; the count pass alone."""
        n, live = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.crdt_count_since(self._ctx, int(n_rows), int(since), ctypes.byref(n),
                                               ctypes.byref(live)), "crdt_count_since")
        return n.value, live.value

    def export_release(self):
        self._check(self._lib.crdt_export_release(self._ctx), "crdt_export_release")

    def merge_from(self, src: "DeviceTable", n_rows: int, since: int, wall: int, win_flags=True):
        """``self.merge(src.recordMap(modifiedSince))`` between two tables of one device and one id
        space: src's export is merged as ONE device changeset, nothing crossing to the host.
        Returns (result dict, win flags) as ``merge`` does for a device batch."""
        self._on_device((src,), "merge_from", "the source")
        ex = src.export_since(n_rows, since)
        offs = np.array([0, ex.n], np.uint64)
        v = ex._view
        b = CrdtBatch(v.key_id, v.lt, v.rank, v.val, None, offs.ctypes.data_as(ctypes.c_void_p), 1,
                      _capi.CRDT_MEM_DEVICE)
        import torch
        return self._merge_batch(b, ex.n, torch.device("cuda", self.device), wall, win_flags)

    def _on_device(self, tables, method: str, noun: str):
        """Every table of ``tables`` is on this one's device, or ValueError ("<method>: <noun> table is on ...")."""
        for t in tables:
            if t.device != self.device:
                raise ValueError(f"{method}: {noun} table is on device {t.device}, this one on {self.device}")

    def _ctx_array(self, tables, method: str, noun: str, lead=()):
        """The C array of the ctx pointers of ``lead`` then ``tables`` (never of zero length), the ``tables``
        checked by ``_on_device``."""
        self._on_device(tables, method, noun)
        ptrs = [t._ctx.value for t in (*lead, *tables)]
        return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)

    def _row_flags_arg(self, row_flags, n_rows: int):
        """(array to return, pointer, memory kind) of a ``row_flags`` argument of the table calls.  For True the
        array is the ``n_rows`` entries of a new device tensor (never an empty allocation)."""
        flags_arr, fptr, mem = None, None, _capi.CRDT_MEM_DEVICE
        if row_flags is True:
            import torch
            full = torch.zeros(max(n_rows, 1), dtype=torch.uint8, device=torch.device("cuda", self.device))
            torch_ready(full)                           # (its zero fill must not land after the merge)
            fptr = ctypes.c_void_p(full.data_ptr())
            flags_arr = full[:n_rows]
        elif row_flags is not None and row_flags is not False:
            flags_arr = row_flags
            if _is_torch(row_flags):
                if not row_flags.is_cuda or row_flags.numel() < n_rows:
                    raise ValueError("row_flags must be a CUDA uint8 tensor of one entry per row")
                fptr = self._dptr(row_flags, "u1", "row_flags")
            else:
                if row_flags.dtype != np.uint8 or not row_flags.flags.c_contiguous or len(row_flags) < n_rows:
                    raise ValueError("row_flags must be a contiguous uint8 array of one entry per row")
                fptr = row_flags.ctypes.data_as(ctypes.c_void_p)
                mem = _capi.CRDT_MEM_HOST
        return flags_arr, fptr, mem

    def merge_table(self, src: "DeviceTable", n_rows: int, since: int, wall: int, row_flags=False):
        """``self.merge(src.recordMap(modifiedSince))`` as ``merge_from`` computes it, in two streaming
        passes over the two tables and without an export (``crdt_merge_table``).  Returns (result dict,
        row flags or None): the flags are indexed by ROW id, one byte for each of ``n_rows`` rows, 1 where
        this table's row was stored.  ``row_flags``: True -> a torch uint8 tensor on the table's device;
        a torch uint8 CUDA tensor -> filled in place; a numpy uint8 array -> host memory, filled in place;
        False/None -> not produced."""
        self._on_device((src,), "merge_table", "the source")
        n_rows = int(n_rows)
        flags_arr, fptr, mem = self._row_flags_arg(row_flags, n_rows)
        res = CrdtResult()
        st = self._lib.crdt_merge_table(self._ctx, src._ctx, n_rows, int(since), int(wall), fptr, mem,
                                        ctypes.byref(res))
        self._check(st, "crdt_merge_table")
        return res.as_dict(), flags_arr

    def sync_tables(self, other: "DeviceTable", n_rows: int, since_self: int, since_other: int, wall: int,
                    row_flags=False):
        """The two-replica exchange ``self.merge(other.recordMap(modifiedSince: since_other))`` then
        ``other.merge(self.recordMap(modifiedSince: since_self))``, both decided on one read of the two
        tables (``crdt_sync_tables``); exactly what the two ``merge_table`` calls leave, the second skipped
        when the first raises.  Returns ((result of self, its row flags), (result of other, its row flags)).
        ``row_flags``: as ``merge_table``'s, or a pair (for self, for other) of arrays of one memory kind."""
        self._on_device((other,), "sync_tables", "the other")
        n_rows = int(n_rows)
        rf_self, rf_other = row_flags if isinstance(row_flags, (tuple, list)) else (row_flags, row_flags)
        arr_a, ptr_a, mem_a = self._row_flags_arg(rf_self, n_rows)
        arr_b, ptr_b, mem_b = self._row_flags_arg(rf_other, n_rows)
        if ptr_a is not None and ptr_b is not None and mem_a != mem_b:
            raise ValueError("sync_tables: both row_flags arrays must live in the same memory (host or device)")
        mem = mem_a if ptr_a is not None else mem_b
        res_a, res_b = CrdtResult(), CrdtResult()
        st = self._lib.crdt_sync_tables(self._ctx, other._ctx, n_rows, int(since_self), int(since_other), int(wall),
                                        ptr_a, ptr_b, mem, ctypes.byref(res_a), ctypes.byref(res_b))
        self._check(st, "crdt_sync_tables")
        return (res_a.as_dict(), arr_a), (res_b.as_dict(), arr_b)

    def merge_tables(self, srcs, n_rows: int, sinces, wall: int, win_mask=False):
        """The hub: ``for s, since in zip(srcs, sinces): self.merge(s.recordMap(modifiedSince: since))`` for up
        to ``_capi.FANIN_MAX`` source tables, decided on one read of this table (``crdt_fanin_tables``); exactly
        what the ``merge_table`` calls leave, the sequence ending at the first that raises.  Returns (list of
        result dicts, one per source; mask or None): ``mask[i]`` has bit j set where merge j stored row i.
        ``win_mask``: as ``merge_table``'s ``row_flags``."""
        return self._fan_tables("merge_tables", "crdt_fanin_tables", "source", srcs, n_rows, sinces, wall, win_mask)

    def _fan_tables(self, method: str, entry: str, noun: str, tables, n_rows: int, sinces, wall: int, win_mask):
        """``merge_tables`` / ``fanout_tables``: this table against ``tables`` (the ``noun`` tables) through the
        C entry point ``entry``."""
        tables, sinces = list(tables), [int(s) for s in sinces]
        if len(sinces) != len(tables):
            raise ValueError(f"{method}: {len(tables)} {noun}s but {len(sinces)} sinces")
        n_rows, n = int(n_rows), len(tables)
        ctxs = self._ctx_array(tables, method, f"a {noun}")
        mask_arr, mptr, mem = self._row_flags_arg(win_mask, n_rows)
        since_arr = (ctypes.c_int64 * max(n, 1))(*sinces)
        res = (CrdtResult * max(n, 1))()
        st = getattr(self._lib, entry)(self._ctx, ctxs, since_arr, n, n_rows, int(wall), mptr, mem, res)
        self._check(st, entry)
        return [res[j].as_dict() for j in range(n)], mask_arr

    def fanout_tables(self, dsts, n_rows: int, sinces, wall: int, win_mask=False):
        """The hub's outbound half, called on the SOURCE: ``for d, since in zip(dsts, sinces):
        d.merge(self.recordMap(modifiedSince: since))`` for up to ``_capi.FANOUT_MAX`` destination tables,
        decided on one read of this table (``crdt_fanout_tables``); exactly what the ``merge_table`` calls leave,
        the sequence ending at the first that raises.  Returns (list of result dicts, one per destination; mask
        or None): ``mask[i]`` has bit j set where destination j stored row i.  ``win_mask``: as
        ``merge_table``'s ``row_flags``."""
        return self._fan_tables("fanout_tables", "crdt_fanout_tables", "destination", dsts, n_rows, sinces, wall,
                                win_mask)

    def diff_table(self, other: "DeviceTable", n_rows: int, flags=False):
        """The read-only comparison of this replica (a) with ``other`` (b) over rows [0, n_rows)
        (``crdt_diff_tables``): neither table, clock, export view or plan is touched.  Returns (dict of
        ``n_a_ahead, n_b_ahead, n_conflict, n_visible_a, n_visible_b, first_diff``; flags or None): the flags
        hold one byte per ROW id, ``_capi.DIFF_A_AHEAD`` where this table holds the winning record,
        ``DIFF_B_AHEAD`` where ``other`` does, ``DIFF_CONFLICT`` where both hold one (lt, rank) with different
        values, and feed ``export_flagged``.  ``flags``: as ``merge_table``'s ``row_flags``."""
        self._on_device((other,), "diff_table", "the other")
        n_rows = int(n_rows)
        flags_arr, fptr, mem = self._row_flags_arg(flags, n_rows)
        d = _capi.CrdtDiff()
        self._check(self._lib.crdt_diff_tables(self._ctx, other._ctx, n_rows, fptr, mem, ctypes.byref(d)),
                    "crdt_diff_tables")
        return d.as_dict(), flags_arr

    def digest_rows(self, n_rows: int, block_rows: int = 1 << 20, state: bool = False) -> np.ndarray:
        """One uint64 word per ``block_rows`` rows of [0, n_rows), computed on the device
        (``crdt_digest_rows``).  ``state=False``: every row as stored, the words of ``bench.row_digests`` at
        the default block.  ``state=True``: what ``Record ==`` sees (invisible rows count for nothing, ``mod``
        is left out), equal for two replicas whenever ``diff_table`` reports no difference."""
        n_rows, block_rows = int(n_rows), int(block_rows)
        if block_rows <= 0:
            raise CrdtNativeError(_capi.CRDT_E_INVALID, "crdt_digest_rows")
        out = np.zeros(-(-n_rows // block_rows) if n_rows > 0 else 0, np.uint64)
        kind = _capi.DIGEST_STATE if state else _capi.DIGEST_ROWS
        self._check(self._lib.crdt_digest_rows(self._ctx, n_rows, block_rows, kind,
                                               out.ctypes.data_as(ctypes.c_void_p), _capi.CRDT_MEM_HOST),
                    "crdt_digest_rows")
        return out

    def clear_rows(self, first: int, count: int):
        self._check(self._lib.crdt_clear_rows(self._ctx, first, count), "crdt_clear_rows")

    def remap_ranks(self, n_rows: int, old_to_new):
        lut = np.ascontiguousarray(old_to_new, dtype=np.uint32)
        self._check(self._lib.crdt_remap_ranks(self._ctx, n_rows, lut.ctypes.data_as(ctypes.c_void_p),
                                               len(lut)), "crdt_remap_ranks")

    def refresh_canonical(self, n_rows: int) -> int:
        v = ctypes.c_int64()
        self._check(self._lib.crdt_refresh_canonical(self._ctx, n_rows, ctypes.byref(v)),
                    "crdt_refresh_canonical")
        return v.value

    # ---------------------------------------------------------------- Crdt API
    def put_stamped(self, key, val, wall: int) -> dict:
        c = _Cols(self.device, key=(key, "u4"), val=(val, "u4"))
        res = CrdtResult()
        self._check(self._lib.crdt_put_stamped(self._ctx, c.ptrs["key"], c.ptrs["val"], len(key), int(wall),
                                               c.mem, ctypes.byref(res)), "crdt_put_stamped")
        return res.as_dict()

    def tombstone_live(self, n_rows: int, wall: int, row_flags=False):
        """``clear()`` on the table (``crdt_tombstone_live``): one ``Hlc.send`` at ``wall``, then every live row
        of [0, n_rows) (visible and not a tombstone) becomes the tombstone ``{C, local rank, null, C}``, in one
        pass over the table; exactly what ``export_since(n_rows, 0)``, a filter on ``val`` and ``put_stamped``
        of the live ids leave, this table's export view untouched.  No live row: nothing moves, whatever the
        wall.  Returns (result dict, row flags or None): the flags are indexed by ROW id, one byte for each of
        ``n_rows`` rows, 1 where the row was tombstoned (they feed ``export_flagged`` on this table).
        ``row_flags``: as ``merge_table``'s."""
        n_rows = int(n_rows)
        flags_arr, fptr, mem = self._row_flags_arg(row_flags, n_rows)
        res = CrdtResult()
        st = self._lib.crdt_tombstone_live(self._ctx, n_rows, int(wall), fptr, mem, ctypes.byref(res))
        self._check(st, "crdt_tombstone_live")
        return res.as_dict(), flags_arr

    def purge_tombstones(self, others, n_rows: int, before: int, row_flags=False):
        """Tombstone collection (``crdt_purge_tombstones``) over this table (member 0) and up to
        ``_capi.PURGE_MAX - 1`` ``others`` of its device and id space; ``others=()`` is one table collecting
        its own.  A row of [0, n_rows) is a candidate iff this table holds it as a visible tombstone with
        ``lt < before`` (signed, strict), and purged iff every member holds a visible tombstone of the same
        (lt, rank); a member that holds the row invisibly blocks it.  A purged row becomes the never-written
        fill in every member (what ``clear_rows(i, 1)`` writes); nothing else, no canonical and no export view
        is touched.  Returns ({"n_candidates", "n_purged"}, row flags or None): the flags are indexed by ROW
        id, one byte for each of ``n_rows`` rows, 1 where the row was purged (they feed ``export_flagged`` on
        any member).  ``row_flags``: as ``merge_table``'s."""
        ctxs = self._ctx_array(list(others), "purge_tombstones", "a member", lead=(self,))
        n_rows = int(n_rows)
        flags_arr, fptr, mem = self._row_flags_arg(row_flags, n_rows)
        out = _capi.CrdtPurge()
        st = self._lib.crdt_purge_tombstones(ctxs, len(ctxs), n_rows, int(before), fptr, mem, ctypes.byref(out))
        self._check(st, "crdt_purge_tombstones")
        return out.as_dict(), flags_arr

    def diff_group(self, others, n_rows: int, masks=False):
        """The read-only comparison of this table (member 0) and up to ``_capi.GROUP_MAX - 1`` ``others`` of its
        device and id space over rows [0, n_rows) (``crdt_diff_group``), every table read once and none written;
        ``others=()`` is one table on its own.  Per row, with a member visible iff its ``mod >= 0``: ``hold`` has
        bit j set where member j holds the greatest (lt, rank) among the visible members, ``behind`` bit j where
        some member holds the row and j's hold bit is clear, ``conflict`` is 1 where two holders carry different
        value handles; a row nobody holds has three zero bytes.  Returns (dict, behind, hold, conflict): the dict
        has ``n_held, n_disputed, n_conflict, first_diff`` and the lists ``n_visible, n_behind, n_sole`` of
        ``GROUP_MAX`` entries (zero from the member count on); the arrays hold one byte per ROW id and feed
        ``export_flagged``.  ``masks``: False/None -> no array (three ``None``); True -> three torch uint8 tensors
        on the table's device; a triple (behind, hold, conflict) whose entries are each as ``merge_table``'s
        ``row_flags``, the arrays that are passed all in one memory (host or device)."""
        ctxs = self._ctx_array(list(others), "diff_group", "a member", lead=(self,))
        n_rows = int(n_rows)
        want = tuple(masks) if isinstance(masks, (tuple, list)) else (masks,) * 3
        if len(want) != 3:
            raise ValueError("diff_group: masks is True, False or a triple (behind, hold, conflict)")
        args = [self._row_flags_arg(m, n_rows) for m in want]
        mems = {mem for _, ptr, mem in args if ptr is not None}
        if len(mems) > 1:
            raise ValueError("diff_group: the mask arrays must live in the same memory (host or device)")
        mem = mems.pop() if mems else _capi.CRDT_MEM_DEVICE
        out = _capi.CrdtGroupDiff()
        st = self._lib.crdt_diff_group(ctxs, len(ctxs), n_rows, args[0][1], args[1][1], args[2][1], mem,
                                       ctypes.byref(out))
        self._check(st, "crdt_diff_group")
        return out.as_dict(), args[0][0], args[1][0], args[2][0]

    def _batch(self, key, lt, rank, val, offsets, millis):
        c = _Cols(self.device, key=(key, "u4"), lt=(lt, "i8"), rank=(rank, "u4"), val=(val, "u4"), millis=(millis, "i8"))
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        c.keep.append(offs)
        b = CrdtBatch(c.ptrs["key"], c.ptrs["lt"], c.ptrs["rank"], c.ptrs["val"], c.ptrs["millis"],
                      offs.ctypes.data_as(ctypes.c_void_p), len(offs) - 1, c.mem)
        return b, c, offs

    def merge(self, key, lt, rank, val, offsets, wall: int, millis=None, win_flags=True):
        """R sequential merges (one per changeset); returns (result dict, win flags or None).

        ``win_flags``: True -> a host uint8 array is returned; a torch uint8 CUDA tensor
        -> filled in place (device batches); False/None -> not produced."""
        b, c, offs = self._batch(key, lt, rank, val, offsets, millis)
        dev = c.keep[0].device if c.mem == _capi.CRDT_MEM_DEVICE else None
        return self._merge_batch(b, int(offs[-1]), dev, wall, win_flags)

    def _merge_batch(self, b, n: int, torch_device, wall: int, win_flags):
        """crdt_merge of a built batch of n records; ``torch_device``: where a device batch's flags go
        (None for a host batch)."""
        flags_arr = None
        fptr = None
        if win_flags is True:
            if torch_device is not None:
                import torch
                flags_arr = torch.zeros(max(n, 1), dtype=torch.uint8, device=torch_device)
                torch_ready(flags_arr)                  # (its zero fill must not land after the merge)
                fptr = ctypes.c_void_p(flags_arr.data_ptr())
            else:
                flags_arr = np.zeros(max(n, 1), np.uint8)
                fptr = flags_arr.ctypes.data_as(ctypes.c_void_p)
        elif win_flags is not None and win_flags is not False:
            flags_arr = win_flags
            if _is_torch(win_flags):
                fptr = self._dptr(win_flags, "u1", "win_flags")
            else:
                if win_flags.dtype != np.uint8 or not win_flags.flags.c_contiguous or len(win_flags) < n:
                    raise ValueError("win_flags must be a contiguous uint8 array of one entry per record")
                fptr = win_flags.ctypes.data_as(ctypes.c_void_p)
        res = CrdtResult()
        st = self._lib.crdt_merge(self._ctx, ctypes.byref(b), int(wall), fptr, ctypes.byref(res))
        if st == _capi.CRDT_E_COMM and getattr(self, "_comm", None) is not None and self._comm.error is not None:
            raise CrdtNativeError(st, f"crdt_merge (communicator: {self._comm.error!r})")
        self._check(st, "crdt_merge")
        if flags_arr is not None and win_flags is True:
            flags_arr = flags_arr[:n]
        return res.as_dict(), flags_arr

    # ------------------------------------------ key-sharded replica (comm_path.inc)
    def comm_unique_id(self) -> bytes:
        """crdt_comm_unique_id: the 128 bytes rank 0 hands every rank (RCCL)."""
        buf = (ctypes.c_uint8 * _capi.COMM_ID_BYTES)()
        self._check(self._lib.crdt_comm_unique_id(buf), "crdt_comm_unique_id")
        return bytes(buf)

    def comm_init_rccl(self, n_ranks: int, rank: int, uid: bytes):
        buf = (ctypes.c_uint8 * _capi.COMM_ID_BYTES).from_buffer_copy(uid)
        self._check(self._lib.crdt_comm_init_rccl(self._ctx, n_ranks, rank, buf), "crdt_comm_init_rccl")

    def comm_init_ops(self, n_ranks: int, rank: int, comm):
        """Join a communicator given as a crdt_comm_ops table (``comm.ops()``, e.g. dist.GlooComm)."""
        self._comm = comm                      # the callbacks must outlive the ctx's use of them
        ops = comm.ops()
        st = self._lib.crdt_comm_init_ops(self._ctx, n_ranks, rank, ctypes.byref(ops))
        self._check(st, "crdt_comm_init_ops")
        ms = getattr(self, "_comm_timeout_ms", None)       # (a deadline set before: the transport's bound too)
        if ms is not None and hasattr(comm, "timeout") and comm.timeout is None:
            comm.timeout = ms / 1e3 if ms else None

    def set_comm_timeout(self, ms: int):
        """crdt_set_comm_timeout: a collective merge's deadline in ms (0 = none).  A host transport given
        to comm_init_ops that has a ``timeout`` of its own (dist.GlooComm) gets the same bound per operation."""
        self._check(self._lib.crdt_set_comm_timeout(self._ctx, int(ms)), "crdt_set_comm_timeout")
        self._comm_timeout_ms = int(ms)
        comm = getattr(self, "_comm", None)
        if comm is not None and hasattr(comm, "timeout"):
            comm.timeout = ms / 1e3 if ms else None

    def comm_state(self) -> tuple[int, str]:
        """crdt_comm_state: (0 usable / 1 aborted at the deadline / 2 aborted on a transport error, the phase
        the current or last collective merge is or was in).  Callable from another thread during a merge."""
        st, ph = ctypes.c_int32(), ctypes.c_char_p()
        self._check(self._lib.crdt_comm_state(self._ctx, ctypes.byref(st), ctypes.byref(ph)), "crdt_comm_state")
        return st.value, (ph.value or b"").decode()

    def comm_info(self) -> tuple[int, int]:
        n, r = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.crdt_comm_info(self._ctx, ctypes.byref(n), ctypes.byref(r)), "crdt_comm_info")
        return n.value, r.value

    def comm_free(self):
        self._check(self._lib.crdt_comm_free(self._ctx), "crdt_comm_free")

    def set_presharded(self, on: bool):
        """True: batches hold only records this rank owns, with key = slot (no record exchange)."""
        self._check(self._lib.crdt_set_presharded(self._ctx, 1 if on else 0), "crdt_set_presharded")

    # ---------------------------------------------------------------- timing
    PATHS = {"auto": 0, "gather": 1, "sorted": 2}

    def set_counts(self, exact: bool):
        """crdt_set_counts: per-record n_present / n_won; False lets the sorted path fold each
        bucket in any order (same rows / canonical / status; both counts reported as 2^64 - 1)."""
        self._check(self._lib.crdt_set_counts(self._ctx, 1 if exact else 0), "crdt_set_counts")

    def set_row_bytes(self, row_bytes: int):
        """crdt_set_row_bytes: 24-B rows (default; sorted-path fan-ins) or 32-B rows (gather-path
        streaming). Same results."""
        self._check(self._lib.crdt_set_row_bytes(self._ctx, int(row_bytes)), "crdt_set_row_bytes")

    def reserve_scratch(self, n_records: int):
        """crdt_reserve_scratch: size the sorted path's partition buffers up front."""
        self._check(self._lib.crdt_reserve_scratch(self._ctx, int(n_records)), "crdt_reserve_scratch")

    def set_rank_bound(self, bound: int):
        """crdt_set_rank_bound: every later rank is < bound (0: no promise).  The sorted path then
        needs no pass over the ranks for its packed key's frame."""
        self._check(self._lib.crdt_set_rank_bound(self._ctx, int(bound)), "crdt_set_rank_bound")

    def set_merge_path(self, path: str):
        """'auto' | 'gather' | 'sorted' (crdt_set_merge_path): the strategy of later merges."""
        self._check(self._lib.crdt_set_merge_path(self._ctx, self.PATHS[path]), "crdt_set_merge_path")

    def last_path(self) -> str:
        v = ctypes.c_int(0)
        self._check(self._lib.crdt_last_path(self._ctx, ctypes.byref(v)), "crdt_last_path")
        return {1: "gather", 2: "sorted"}[v.value]

    PLAN_FLAGS = {"sorted": 1, "packed": 2, "two_level": 4, "hist_in_scan": 8, "key8": 16, "key16": 32,
                  "high_water": 64, "anchored": 128, "wire_packed": 256, "own_in_place": 512,
                  "flagged": 1024, "ordered": 2048,
                  "combined": 4096, "route_l1": 8192, "route_tuned": 16384, "rl1_head": 262144,
                  "compact": 524288, "hot_direct": 1048576, "table": 2097152,
                  "sync": 4194304, "fanin": 8388608, "fanout": 16777216}

    def last_plan(self) -> dict:
        """crdt_last_plan: how the last merge ran ({'sorted': bool, 'packed': ..., ...})."""
        v = ctypes.c_uint32(0)
        self._check(self._lib.crdt_last_plan(self._ctx, ctypes.byref(v)), "crdt_last_plan")
        plan = {k: bool(v.value & b) for k, b in self.PLAN_FLAGS.items()}
        plan["rl1_pieces"] = (v.value >> 15) & 7                # route_l1's pipelined pieces (0: not route_l1)
        return plan

    def place_info(self) -> dict:
        """crdt_place_info: the level-1 placement tuner ({'candidates': n, 'kept': index or None while the
        trials run, 'merges_used': the warm-up + two merges per candidate so far, 'level1_ms': each candidate's
        timed level-1 scatter, the faster of its two trials})."""
        n, kept, done = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        ms = (ctypes.c_float * 4)()
        self._check(self._lib.crdt_place_info(self._ctx, ctypes.byref(n), ctypes.byref(kept), ctypes.byref(done), ms),
                    "crdt_place_info")
        return {"candidates": n.value, "kept": kept.value if kept.value >= 0 else None, "merges_used": done.value,
                "level1_ms": [round(float(m), 3) for m in ms[:max(n.value, 0)]]}

    TUNE_WAYS = ("route_l1", "combine", "route_l1_4", "route_l1_1", "route_l1_head")

    def route_tune(self) -> dict:
        """crdt_route_tune_info: the sharded fan-in routing the ctx measured ({'best': None while the
        trials run, else 'route_l1' (2 pipelined pieces) / 'combine' / 'route_l1_4' (4) / 'route_l1_1' (1) /
        'route_l1_head' (2 pieces, the owners' first digit folded at the sender); '<way>_ms': each way's timed
        call, max over ranks, None if not yet})."""
        best = ctypes.c_int32(0)
        us = (ctypes.c_int64 * 5)()
        self._check(self._lib.crdt_route_tune_info(self._ctx, ctypes.byref(best), us), "crdt_route_tune_info")
        out = {"best": self.TUNE_WAYS[best.value] if 0 <= best.value < len(self.TUNE_WAYS) else None}
        for w, u in zip(self.TUNE_WAYS, us):
            out[f"{w}_ms"] = u / 1e3 if u >= 0 else None
        return out

    def set_timing(self, enable: bool):
        self._check(self._lib.crdt_set_timing(self._ctx, int(bool(enable))), "crdt_set_timing")

    def timing(self) -> dict:
        t = CrdtTiming()
        self._check(self._lib.crdt_get_timing(self._ctx, ctypes.byref(t)), "crdt_get_timing")
        return t.as_dict()
