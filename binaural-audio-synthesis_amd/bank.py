"""HRTF table banks: many tables of one shape side by side on the device, a table per session or per batch item
(include/bas_bank.h).

A bank holds T tables of the same ndir, M and upsampling (U >= 4) in two allocations,
    packed [T][2][ndir][U][L + 4] float32   each slice what bas_table_pack_f32 writes for that table, guards included,
    diffs  [T][2][ndir][ndir]     float64,
and a render picks the table per chunk-boundary COLUMN of its angle rows: `table_of`, int32 [cols].  The plan kernel adds
table t's base to the 16 byte offsets of a read plan, and every FIR kernel - which only ever adds those offsets to one buffer
resource over `packed` - serves the bank unchanged.  Two callers take a bank: StreamBatchRenderer (a table per session) and
render_batch (a table per item); every other interface refuses one (apply_hrtf.as_device_table).

The shape rules (`bank_shape`), the size limit (`bank_bytes`, MAX_BANK_BYTES), the validation of table indices
(`check_tables`) and the layout -> columns step (`stream_table_columns`, `batch_table_columns`) are plain numpy and need no GPU.
"""
import numpy as np

from . import _hip

PLANE_GUARDS = 4                 # floats a phase plane holds beside its L samples (BAS_PLANE of csrc/bas_plan.h)
MIN_UPSAMPLING = 4               # the read plans' form (BAS_PLAN_MIN_U); banks do not take the plain U < 4 kernel
MAX_BANK_BYTES = 1 << 31         # the whole of `packed` stays BELOW this: one buffer resource, 32-bit byte offsets


def table_bytes(ndir, L, U):
    """Bytes of one packed table: 2 ears x ndir x U planes of L + 4 floats."""
    return 2 * int(ndir) * int(U) * (int(L) + PLANE_GUARDS) * 4


def bank_bytes(n_tables, ndir, L, U):
    """Bytes of the packed tables of a bank (must stay below MAX_BANK_BYTES)."""
    return int(n_tables) * table_bytes(ndir, L, U)


def max_tables(ndir, L, U):
    """The largest bank of tables of this shape: about 1300 at L = 128, U = 8, about 340 at L = 512."""
    return (MAX_BANK_BYTES - 1) // table_bytes(ndir, L, U)


def bank_shape(tables):
    """(T, ndir, M, U) of a sequence of tables (device tables or structs with the reference's five attributes), or
    ValueError: an empty sequence, a table whose fields disagree among themselves, tables that disagree in ndir, M or
    upsampling, upsampling < 4, a bank of 2^31 bytes or more.  Shapes only: no array is read, nothing is allocated."""
    tables = list(tables)
    if not tables:
        raise ValueError("a bank needs at least one table")
    first, seen = None, set()
    for t, tbl in enumerate(tables):
        if id(tbl) in seen:                               # (the same object again: checked already)
            continue
        seen.add(id(tbl))
        U = int(tbl.upsampling)
        il, ir = tuple(np.shape(tbl.irs_left)), tuple(np.shape(tbl.irs_right))
        if il != ir or len(il) != 2 or U <= 0 or il[1] % U:
            raise ValueError(f"table {t}: irs_left/irs_right must be (ndir, samples_to_keep*upsampling)")
        ndir, M = il
        if tuple(np.shape(tbl.diffs_left)) != (ndir, ndir) or tuple(np.shape(tbl.diffs_right)) != (ndir, ndir):
            raise ValueError(f"table {t}: diffs_left/diffs_right must be (ndir, ndir)")
        if ndir == 0 or M == 0:
            raise ValueError(f"table {t} is empty")
        if first is None:
            first = (ndir, M, U)
        elif (ndir, M, U) != first:
            raise ValueError(f"table {t} has (ndir, M, upsampling) = {(ndir, M, U)}, table 0 has {first}: the tables of "
                             f"a bank must agree in all three")
    ndir, M, U = first
    if U < MIN_UPSAMPLING:
        raise ValueError(f"banks need an upsampling factor >= {MIN_UPSAMPLING} (the read plans' form), got {U}")
    T = len(tables)
    if bank_bytes(T, ndir, M // U, U) >= MAX_BANK_BYTES:
        raise ValueError(f"a bank of {T} tables of {table_bytes(ndir, M // U, U)} bytes is {bank_bytes(T, ndir, M // U, U)} "
                         f"bytes: it must stay below 2^31 (at most {max_tables(ndir, M // U, U)} tables of this shape)")
    return T, ndir, M, U


def check_tables(tables, n, n_tables, what):
    """Host table indices, one per `what` (session, item), as an int32 numpy array [n]: ValueError for another length,
    values that are not whole numbers or values outside [0, n_tables)."""
    arr = np.asarray(tables)
    if arr.shape != (int(n),):
        raise ValueError(f"tables must hold one table index per {what} ({n}), got shape {arr.shape}")
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        if not (np.issubdtype(arr.dtype, np.floating) and np.isfinite(arr).all() and (arr == np.floor(arr)).all()):
            raise ValueError("table indices must be whole numbers")
    if arr.size and (arr.min() < 0 or arr.max() >= n_tables):
        raise ValueError(f"table indices must lie in [0, {n_tables}), got {int(arr.min())} .. {int(arr.max())}")
    return arr.astype(np.int32)


def stream_table_columns(lay, tables):
    """int32 [lay.n_q]: the table of every chunk-boundary column of a StreamLayout - session g's index on all of its
    nh + nb columns (the carried halo's, the block's; the gap chunk's two boundaries are the last of g and the first of
    g + 1)."""
    return np.repeat(np.asarray(tables, dtype=np.int32), lay.nh + lay.nb)


def batch_table_columns(lay, tables):
    """int32 [lay.n_q]: the table of every chunk-boundary column of a batch Layout - item b's index on its own
    T_in_b/K + 1 columns and on the filler columns behind it (their inputs are zero: the index only has to be legal)."""
    first = np.append(lay.q_offsets, lay.n_q)
    return np.repeat(np.asarray(tables, dtype=np.int32), np.diff(first))


class TableBank:
    """T tables of one shape on the device (module docstring).  tables: a non-empty sequence of device tables
    (irs_and_delaydiffs) or objects with the reference's five attributes; the same object may appear more than once (it
    is uploaded once and packed into each of its slices).  Every shape check runs before any device work (ValueError)."""

    def __init__(self, tables, device=None):
        import torch
        from .apply_hrtf import irs_and_delaydiffs
        tables = list(tables)
        self.n_tables, self.ndir, self.M, self.upsampling = bank_shape(tables)
        self.L = self.M // self.upsampling
        device = _hip.require_gpu(device)
        self.device = device
        T, ndir, M, U = self.n_tables, self.ndir, self.M, self.upsampling
        lib = _hip.lib()
        per_table = lib.bas_table_packed_floats(ndir, M, U)
        assert per_table * 4 == table_bytes(ndir, self.L, U)
        self.packed = torch.empty((T, per_table), dtype=torch.float32, device=device)   # [T][2][ndir][U][L + 4]
        self.diffs = torch.empty((T, 2, ndir, ndir), dtype=torch.float64, device=device)
        staged = {}                                       # id(table) -> its [2][ndir][M] float32 device copy
        with _hip.on_device(device):
            stream = _hip.current_stream(device)
            for t, tbl in enumerate(tables):
                if id(tbl) not in staged:
                    if isinstance(tbl, irs_and_delaydiffs):
                        irs = torch.stack([tbl.irs_left, tbl.irs_right]).to(device)
                        diffs = tbl.diffs.to(device)
                    else:
                        irs = torch.from_numpy(np.stack([np.ascontiguousarray(tbl.irs_left, dtype=np.float32),
                                                         np.ascontiguousarray(tbl.irs_right, dtype=np.float32)])).to(device)
                        diffs = torch.from_numpy(np.stack([np.ascontiguousarray(tbl.diffs_left, dtype=np.float64),
                                                           np.ascontiguousarray(tbl.diffs_right, dtype=np.float64)])).to(device)
                    staged[id(tbl)] = (irs, diffs)
                irs, diffs = staged[id(tbl)]
                self.diffs[t].copy_(diffs)
                _hip.call("bas_table_pack_f32", _hip.ptr(irs), ndir, M, U, _hip.ptr(self.packed[t]), stream)

    @property
    def ndir_all(self):
        """What the FIR entry points take as ndir with the bank's `packed`: there it only sizes the table resource."""
        return self.n_tables * self.ndir


def table_columns_to_device(bank, table_of, cols=None, n_q=None):
    """A caller's table_of for `bank`: a contiguous int32 tensor on the bank's device, of `cols` entries when cols is
    given, else of a length that divides n_q (ValueError otherwise).  Values are not read (the kernel clamps them)."""
    import torch
    if not (isinstance(table_of, torch.Tensor) and table_of.is_cuda and table_of.dtype == torch.int32
            and table_of.dim() == 1 and table_of.is_contiguous() and table_of.device == bank.device):
        raise ValueError("table_of must be a contiguous one-dimensional int32 tensor on the bank's device")
    n = table_of.numel()
    if cols is not None and n != cols:
        raise ValueError(f"table_of must hold one table index per chunk-boundary column ({cols}), got {n}")
    if cols is None and (n == 0 or n_q % n):
        raise ValueError(f"table_of holds {n} columns, which does not divide the {n_q} queries")
    return table_of
