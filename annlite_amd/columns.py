"""Filterable columns on the device: the declared ``columns`` of an ``AnnLite`` as typed device arrays of the row range, and the
filter dict compiled to the predicate program ``annlite_filter_eval`` runs over them.

The reference keeps its declared columns in a SQLite cell table and turns the filter into a WHERE clause over them
(annlite/storage/table.py: ``CellTable.query``); what comes out are the offsets the index is given as ``indices``.  Here

  * ``ColumnStore`` holds one array per declared column -- ``I64`` (``int`` / ``bool``), ``F64`` (``float``) or ``CODE`` (``str``: an
    i32 code into a per-column dictionary) --, one present bit per row and column, and one row-present bit per row;
  * ``ColumnStore.compile`` is the symbolic twin of ``filter._tokens`` / ``filter._reduce``: the same grammar, the same splice into
    one flat clause, the same errors -- but its operands are leaves over columns instead of booleans, and what it returns is a
    postfix program (or ``None``: the host evaluates the filter, as before);
  * ``ColumnStore.evaluate`` launches the kernel and returns a ``RowMask``: the packed words a search takes as its bitmap;
  * ``ColumnStore.page`` selects one page of the document listing (``AnnLite.filter`` / ``get_docs``: ``order_by``, ``offset``,
    ``limit``) on the device -- a radix select over ``order_key`` of a regular column, ``annlite_order_page`` -- and brings only the
    page's offsets to the host.

The rule that keeps the answer equal to Python's: only values and literals whose comparison the kernel reproduces EXACTLY are taken
(8-byte integers against 8-byte integers, doubles against doubles, every mixed case lowered by the table in ``_lower_i64``); anything
else -- a NaN, a str in a numeric column, an int beyond int64, a numpy scalar as a literal -- makes the column *irregular* or the
filter uncompiled, and Python answers.
"""
import ctypes
import math
import numbers
import struct
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _capi
from .filter import _COMPARE, _LOGIC, _MEMBER, _compare, _unsupported

I64, F64, CODE = _capi.COL_I64, _capi.COL_F64, _capi.COL_CODE
OP_LT, OP_GT, OP_LE, OP_GE, OP_EQ, OP_NE, OP_IN, OP_NIN, OP_IN_SET = range(9)
CODE_AND, CODE_OR, CODE_NOT, CODE_TRUE = 0x80, 0x81, 0x82, 0x83
MAX_LEAVES, MAX_LITERALS, MAX_CODE, MAX_STACK = (_capi.FILTER_MAX_LEAVES, _capi.FILTER_MAX_LITERALS, _capi.FILTER_MAX_CODE,
                                                 _capi.FILTER_MAX_STACK)
MAX_STRINGS = 65536  # distinct values of one str column; the next one makes the column irregular
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
EXACT_F64_INT = 2 ** 53  # |v| <= 2^53: the integers a double holds exactly, one after the other

_OPS = {'$lt': OP_LT, '$gt': OP_GT, '$lte': OP_LE, '$gte': OP_GE, '$eq': OP_EQ, '$neq': OP_NE, '$ne': OP_NE, '$in': OP_IN, '$nin': OP_NIN}
_TORCH = {I64: torch.int64, F64: torch.float64, CODE: torch.int32}
_NUMPY = {I64: np.int64, F64: np.float64, CODE: np.int32}
_NEVER, _ALWAYS = (OP_GT, INT64_MAX), (OP_LE, INT64_MAX)  # over i64 values: no row / every row that has the value


def column_kind(dtype) -> Optional[int]:
    """The device kind of a declared column type (the reference's SQL types: INTEGER, FLOAT, TEXT), None for any other (BLOB ...)."""
    if isinstance(dtype, str):
        return {'integer': I64, 'float': F64, 'text': CODE}.get(dtype.lower())
    if not isinstance(dtype, type):
        return None
    if dtype is str:
        return CODE
    if dtype is float or issubclass(dtype, np.floating):
        return F64
    if dtype in (int, bool) or issubclass(dtype, np.integer):
        return I64
    return None


def n_words_of(capacity: int) -> int:
    """words of a row bitmap over ``capacity`` rows: the indexes' layout, two spare words behind the rows"""
    return (capacity + 31) // 32 + 2


def _lower_i64(op: int, c: float):
    """``x op c`` for an int64 ``x`` and a float ``c`` (not NaN) as ``x op' t`` with an int64 ``t``: Python compares an int with a float
    exactly, so  x < c <=> x < ceil(c),  x <= c <=> x <= floor(c),  x > c <=> x > floor(c),  x >= c <=> x >= ceil(c),  x == c <=> c is
    integral and x == int(c); a bound outside int64 (the infinities too) folds to every row / no row."""
    if op in (OP_EQ, OP_NE):
        if math.isinf(c) or c != math.floor(c) or not INT64_MIN <= int(c) <= INT64_MAX:
            return _NEVER if op == OP_EQ else _ALWAYS
        return op, int(c)
    up = op in (OP_LT, OP_GE)  # (the bound rounds up)
    if math.isinf(c):
        t = INT64_MAX + 1 if c > 0 else INT64_MIN - 1
    else:
        t = math.ceil(c) if up else math.floor(c)
    if t > INT64_MAX:
        return _ALWAYS if op in (OP_LT, OP_LE) else _NEVER
    if t < INT64_MIN:
        return _NEVER if op in (OP_LT, OP_LE) else (OP_GE, INT64_MIN)
    return op, t


PAGE_MAX = _capi.PAGE_MAX  # rows of one page taken on the device
_U64 = 2 ** 64 - 1


def order_key(kind: int, value) -> int:
    """The value of a regular column as the 64-bit unsigned key the page kernels order by (``annlite_order_page``): ``key(a) < key(b)``
    exactly where Python has ``a < b``, equal keys where it has ``a == b``.  ``I64``: ``x ^ 2**63`` over the int64 (``True`` is 1);
    ``F64``: the monotone flip of the double's bits, -0.0 first made +0.0 (ints in the column are the doubles that hold them
    exactly); ``CODE``: the value is the word's rank in the sorted dictionary already (``rank_table``).  Descending order is by
    ``~key``."""
    if kind == I64:
        return (int(value) & _U64) ^ (1 << 63)
    if kind == F64:
        u = struct.unpack('<Q', struct.pack('<d', float(value)))[0]
        if (u << 1) & _U64 == 0:  # (-0.0 == 0.0)
            u = 0
        return u ^ (_U64 if u >> 63 else 1 << 63)
    assert kind == CODE, kind
    return int(value)


def rank_table(words: Sequence[str]) -> np.ndarray:
    """i32 [len(words)]: code (the position in ``words``, a column's dictionary in insertion order) -> the word's position in
    ``sorted(words)`` -- Python's order of str, by code point."""
    rank = np.zeros((len(words),), dtype=np.int32)
    rank[sorted(range(len(words)), key=words.__getitem__)] = np.arange(len(words), dtype=np.int32)
    return rank


class Leaf:
    __slots__ = ('column', 'kind', 'op', 'lit_begin', 'lit_count', 'set_bits')

    def __init__(self, column: str, kind: int, op: int, lit_begin: int = 0, lit_count: int = 0, set_bits: Optional[np.ndarray] = None):
        self.column, self.kind, self.op, self.lit_begin, self.lit_count, self.set_bits = column, kind, op, lit_begin, lit_count, set_bits


class Program:
    """A compiled filter: ``leaves`` (column, op, literal range), ``literals`` (ints for I64 leaves, floats for F64 leaves), the postfix
    ``code`` (bytes: 0 .. 31 push a leaf, ``CODE_AND`` / ``CODE_OR`` / ``CODE_NOT`` / ``CODE_TRUE``) and the ``depth`` its stack reaches."""

    def __init__(self, leaves: List[Leaf], literals: List, code: bytes, depth: int):
        self.leaves, self.literals, self.code, self.depth = leaves, literals, code, depth

    def raw_literals(self) -> List[int]:
        """the literal pool as the kernel reads it: raw 8-byte patterns"""
        kind_of = {}
        for leaf in self.leaves:
            for j in range(leaf.lit_begin, leaf.lit_begin + leaf.lit_count):
                kind_of[j] = leaf.kind
        return [struct.unpack('<Q', struct.pack('<d', v) if kind_of.get(j) == F64 else struct.pack('<q', v))[0]
                for j, v in enumerate(self.literals)]


class _Uncompiled(Exception):
    pass


class _Compiler:
    """``filter._tokens`` over leaves: the tokens are 'AND' / 'OR' and expression nodes -- ('leaf', i), ('true',), ('not', e),
    ('and', [e ...]), ('or', [e ...]).  A leaf that cannot be lowered clears ``ok`` and the walk goes on: a malformed filter raises what
    ``filter.select`` raises wherever it stands."""

    def __init__(self, store: 'ColumnStore'):
        self.store, self.ok = store, True
        self.leaves: List[Leaf] = []
        self.literals: List = []

    # ---- the grammar (line by line filter._tokens / filter._reduce)
    @staticmethod
    def reduce(tokens: List):
        if not tokens:
            return ('true',)
        groups: List[List] = [[]]
        for tok in tokens:
            if tok == 'OR':
                groups.append([])
            elif tok != 'AND':
                groups[-1].append(tok)
        ands = [('true',) if not g else g[0] if len(g) == 1 else ('and', g) for g in groups]
        return ands[0] if len(ands) == 1 else ('or', ands)

    def tokens(self, data, logic: str = 'AND') -> List:
        out: List = []
        if isinstance(data, dict):
            for i, (key, value) in enumerate(data.items()):
                if key in _LOGIC:
                    if i > 0:
                        out.append(_LOGIC[key])
                    out.extend(self.tokens(value, _LOGIC[key]))
                elif key == '$not':
                    if i > 0:
                        out.append(logic)
                    out.append(('not', self.reduce(self.tokens(value))))
                elif key.startswith('$'):
                    raise _unsupported(key)
                else:
                    if i > 0:
                        out.append(logic)
                    if not isinstance(value, dict):
                        out.append(self.leaf(key, '$eq', value))
                        continue
                    if not value:
                        raise ValueError(f'The query express is illegal: {data}')
                    parts: List = []
                    for op, ref in value.items():
                        if parts:
                            parts.append('AND')
                        if op in _LOGIC:
                            parts.extend(self.tokens(ref, _LOGIC[op]))
                        elif op in _COMPARE or op in _MEMBER:
                            parts.append(self.leaf(key, op, ref))
                        else:
                            raise _unsupported(op)
                    out.extend(parts)
        elif isinstance(data, (list, tuple)):
            inner: List = []
            for d in data:
                if inner:
                    inner.append(logic)
                inner.extend(self.tokens(d))
            out.append(self.reduce(inner))
        else:
            raise ValueError(f'The query express is illegal: {data}')
        return out

    # ---- leaves
    def leaf(self, column: str, op_name: str, ref):
        try:
            return ('leaf', self._leaf(column, op_name, ref))
        except _Uncompiled:
            self.ok = False
            return ('true',)

    def _number(self, kind: int, ref):
        """a literal as the column's own type, exactly -- or uncompiled.  Python's own ``int`` / ``bool`` / ``float`` only: what a numpy
        scalar does in a mixed comparison is numpy's business."""
        if type(ref) in (int, bool):
            if kind == F64:
                if abs(int(ref)) > EXACT_F64_INT:
                    raise _Uncompiled
                return float(ref)
            if not INT64_MIN <= int(ref) <= INT64_MAX:
                raise _Uncompiled
            return int(ref)
        if type(ref) is float and not math.isnan(ref):
            return ref  # (against an I64 column: still a float, lowered by the caller)
        raise _Uncompiled

    def _push(self, values: Sequence):
        begin = len(self.literals)
        if begin + len(values) > MAX_LITERALS:
            raise _Uncompiled
        self.literals.extend(values)
        return begin, len(values)

    def _leaf(self, column: str, op_name: str, ref) -> int:
        store = self.store
        kind = store.kinds.get(column)
        if kind is None or column in store.irregular or len(self.leaves) >= MAX_LEAVES:
            raise _Uncompiled
        op = _OPS[op_name]
        if kind == CODE:
            # Python's own answer per dictionary entry, whatever the operator and the reference value are
            words = store.dictionary(column)
            bits = np.zeros((max(1, (len(words) + 31) // 32) * 32,), dtype=bool)
            try:
                for code, word in enumerate(words):
                    bits[code] = _compare(word, op_name, ref)
            except Exception:
                raise _Uncompiled
            leaf = Leaf(column, kind, OP_IN_SET, set_bits=np.packbits(bits, bitorder='little').view('<u4'))
        elif op in (OP_IN, OP_NIN):
            if not isinstance(ref, (list, tuple, set, frozenset)):
                raise _Uncompiled
            values = []
            for r in ref:
                v = self._number(kind, r)
                if kind == I64 and isinstance(v, float):
                    eq = _lower_i64(OP_EQ, v)
                    if eq == _NEVER:
                        continue  # (equals no integer)
                    v = eq[1]
                if v not in values:
                    values.append(v)
            leaf = Leaf(column, kind, op, *self._push(values))
        else:
            v = self._number(kind, ref)
            if kind == I64 and isinstance(v, float):
                op, v = _lower_i64(op, v)
            leaf = Leaf(column, kind, op, *self._push([v]))
        self.leaves.append(leaf)
        return len(self.leaves) - 1

    # ---- postfix
    def emit(self, node, code: bytearray) -> int:
        """append the node's code; returns the stack depth it needs"""
        tag = node[0]
        if tag == 'leaf':
            code.append(node[1])
            return 1
        if tag == 'true':
            code.append(CODE_TRUE)
            return 1
        if tag == 'not':
            depth = self.emit(node[1], code)
            code.append(CODE_NOT)
            return depth
        depth = self.emit(node[1][0], code)
        for child in node[1][1:]:
            depth = max(depth, 1 + self.emit(child, code))
            code.append(CODE_AND if tag == 'and' else CODE_OR)
        return depth


class RowMask:
    """What a compiled filter evaluates to: ``words`` (i32 [n_words] on the device, bit r = row r passes and is present; every word
    behind the rows 0), ``len()`` -- the number of rows, the one host read -- and ``offsets()``, ascending, made on demand."""

    def __init__(self, words: torch.Tensor, count: torch.Tensor, n_rows: int, keep=()):
        self.words, self.n_rows = words, n_rows
        self._count_dev, self._count, self._keep = count, None, keep

    def __len__(self) -> int:
        if self._count is None:
            self._count = int(self._count_dev.item())
            self._keep = ()
        return self._count

    def words_for(self, n_words: int) -> torch.Tensor:
        """the words as a bitmap of ``n_words`` words (an index whose capacity is not the store's): cut or zero-filled"""
        if self.words.numel() == n_words:
            return self.words
        out = torch.zeros((n_words,), dtype=self.words.dtype, device=self.words.device)
        n = min(n_words, self.words.numel())
        out[:n] = self.words[:n]
        return out

    def flags(self, n: Optional[int] = None) -> torch.Tensor:
        """bool [n] on the device (default: the store's rows); rows beyond the words are False"""
        n = self.n_rows if n is None else n
        words = self.words_for((n + 31) // 32) if n > self.words.numel() * 32 else self.words
        shifts = torch.arange(32, device=words.device, dtype=torch.int32)
        return ((words[:, None] >> shifts[None, :]) & 1).bool().reshape(-1)[:n]

    def offsets(self) -> np.ndarray:
        return torch.nonzero(self.flags()).reshape(-1).cpu().numpy().astype(np.int64, copy=False)


class ColumnStore:
    """The declared columns over the row range ``[0, len)``.  ``append`` adds rows (one tag dict each, None: a row without tags),
    ``drop`` clears row-present bits (deleted documents), ``clear`` forgets everything.  Nothing is allocated before the first rows
    arrive; ``device`` defaults to the current HIP device (``'cpu'``: the arrays as host tensors, for tests of the host side)."""

    def __init__(self, columns, device=None, initial_capacity: int = 10240):
        items = columns.items() if isinstance(columns, dict) else (columns or ())
        self.kinds: Dict[str, int] = {}
        for name, dtype in items:
            kind = column_kind(dtype)
            if kind is not None:  # (a type without a device kind is a tag like any undeclared one: the host answers)
                self.kinds[name] = kind
        self._device = device
        self._initial = max(64, int(initial_capacity))
        self.clear()

    def clear(self):
        self.irregular = set()
        self._n, self._cap = 0, 0
        self.values: Dict[str, torch.Tensor] = {}
        self.present: Dict[str, torch.Tensor] = {}
        self.rows: Optional[torch.Tensor] = None
        self._h_present: Dict[str, np.ndarray] = {}
        self._h_rows: Optional[np.ndarray] = None
        self._codes: Dict[str, Dict[str, int]] = {n: {} for n, k in self.kinds.items() if k == CODE}
        self._ranks: Dict[str, torch.Tensor] = {}  # (per str column: code -> rank in the sorted dictionary, for pages)
        self._workspace = None

    def __len__(self) -> int:
        return self._n

    @property
    def capacity(self) -> int:
        return self._cap

    @property
    def n_words(self) -> int:
        return n_words_of(self._cap)

    def dictionary(self, column: str) -> List[str]:
        return list(self._codes[column])  # (insertion order = code order)

    # ------------------------------------------------------------------ storage
    def _dev(self):
        if self._device is None:
            from . import ops

            self._device = ops.device()
        return torch.device(self._device)

    def _grow(self, need: int):
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, self._initial)
        cap = (cap + 1023) // 1024 * 1024 if cap > 1024 else (cap + 63) // 64 * 64
        dev, W = self._dev(), n_words_of(cap)

        def grown(old, shape, dtype):
            new = torch.zeros(shape, dtype=dtype, device=dev)
            if old is not None:
                new[: old.numel()] = old
            return new

        def grown_host(old):
            new = np.zeros((W,), dtype=np.uint32)
            if old is not None:
                new[: old.size] = old
            return new

        for name, kind in self.kinds.items():
            self.values[name] = grown(self.values.get(name), (cap,), _TORCH[kind])
            self.present[name] = grown(self.present.get(name), (W,), torch.int32)
            self._h_present[name] = grown_host(self._h_present.get(name))
        self.rows = grown(self.rows, (W,), torch.int32)
        self._h_rows = grown_host(self._h_rows)
        self._cap = cap

    def _set_range(self, host: np.ndarray, dev: torch.Tensor, n0: int, flags: np.ndarray):
        """bits [n0, n0 + len) of the host words |= flags; the touched words go to the device"""
        w0, w1 = n0 >> 5, (n0 + flags.size + 31) >> 5
        bits = np.zeros(((w1 - w0) * 32,), dtype=bool)
        bits[n0 - w0 * 32: n0 - w0 * 32 + flags.size] = flags
        host[w0:w1] |= np.packbits(bits, bitorder='little').view('<u4')
        dev[w0:w1] = torch.from_numpy(host[w0:w1].view(np.int32)).to(dev.device)

    def _column_batch(self, name: str, kind: int, tags: Sequence[Optional[dict]]):
        """(values, present) of the batch by the type rule, or None: a value outside the rule (the column turns irregular)"""
        n = len(tags)
        vals = np.zeros((n,), dtype=_NUMPY[kind])
        pres = np.zeros((n,), dtype=bool)
        codes = self._codes.get(name)
        for r, t in enumerate(tags):
            v = t.get(name) if t else None
            if v is None:
                continue  # NULL
            if kind == CODE:
                if not isinstance(v, str):
                    return None
                code = codes.get(v)
                if code is None:
                    if len(codes) >= MAX_STRINGS:
                        return None
                    code = codes[v] = len(codes)
                vals[r] = code
            elif isinstance(v, numbers.Integral):  # (bools included)
                iv = int(v)
                # a numpy integer compares with a float through float64: exact only where the double is
                limit = EXACT_F64_INT if kind == F64 or not isinstance(v, int) else None
                if not INT64_MIN <= iv <= INT64_MAX or (limit is not None and abs(iv) > limit):
                    return None
                vals[r] = iv
            elif kind == F64 and isinstance(v, float) and not math.isnan(v):
                vals[r] = v
            else:
                return None
            pres[r] = True
        return vals, pres

    def append(self, tags: Sequence[Optional[dict]]):
        n = len(tags)
        if n == 0 or not self.kinds:  # (no declared column: no filter compiles, nothing to keep)
            return
        n0 = self._n
        self._grow(n0 + n)
        for name, kind in self.kinds.items():
            if name in self.irregular:
                continue
            batch = self._column_batch(name, kind, tags)
            if batch is None:
                self.irregular.add(name)  # (until clear(): filters that name the column take the host path)
                continue
            vals, pres = batch
            self.values[name][n0: n0 + n] = torch.from_numpy(vals).to(self.values[name].device)
            self._set_range(self._h_present[name], self.present[name], n0, pres)
        self._set_range(self._h_rows, self.rows, n0, np.array([t is not None for t in tags], dtype=bool))
        self._n = n0 + n

    def drop(self, offsets):
        offs = np.asarray(list(offsets), dtype=np.int64).reshape(-1)
        offs = offs[(offs >= 0) & (offs < self._n)]
        if offs.size == 0:
            return
        np.bitwise_and.at(self._h_rows, offs >> 5, ~(np.uint32(1) << (offs & 31).astype(np.uint32)))
        touched = np.unique(offs >> 5)
        self.rows[torch.from_numpy(touched).to(self.rows.device)] = torch.from_numpy(self._h_rows[touched].view(np.int32)).to(self.rows.device)

    # ------------------------------------------------------------------ filters
    def compile(self, flt) -> Optional[Program]:
        """The filter as a program over this store's columns; None where the host has to answer: a field that is not declared or is
        irregular, a literal that cannot be lowered exactly, a limit exceeded.  Raises what ``filter.select`` raises, where it does."""
        comp = _Compiler(self)
        root = comp.reduce(comp.tokens(flt or {}))
        if not comp.ok:
            return None
        code = bytearray()
        depth = comp.emit(root, code)
        if depth > MAX_STACK or len(code) > MAX_CODE:
            return None
        return Program(comp.leaves, comp.literals, bytes(code), depth)

    def bind(self, program: Program):
        """(the C struct, what it points to): the program over this store's device arrays"""
        P = _capi.FilterProgram()
        keep = []
        P.n_leaves, P.n_literals, P.n_code = len(program.leaves), len(program.literals), len(program.code)
        for i, leaf in enumerate(program.leaves):
            L = P.leaves[i]
            L.values_dev = self.values[leaf.column].data_ptr()
            L.present_dev = self.present[leaf.column].data_ptr()
            L.kind, L.op, L.lit_begin, L.lit_count = leaf.kind, leaf.op, leaf.lit_begin, leaf.lit_count
            if leaf.set_bits is not None:
                bits = torch.from_numpy(leaf.set_bits.view(np.int32)).to(self.rows.device)
                keep.append(bits)
                L.set_bits_dev, L.set_words = bits.data_ptr(), bits.numel()
        for j, raw in enumerate(program.raw_literals()):
            P.literals[j] = raw
        ctypes.memmove(P.code, program.code, len(program.code))
        return P, keep

    def evaluate(self, program: Program, max_blocks: int = 0) -> RowMask:
        """``annlite_filter_eval`` over the store's rows, ANDed with the row-present words."""
        from . import ops

        assert self._n > 0, 'no rows: nothing to evaluate'
        P, keep = self.bind(program)
        words, count = ops.filter_eval(P, self._n, self.n_words, and_bits=self.rows, max_blocks=max_blocks)
        return RowMask(words, count, self._n, keep=keep)

    # ------------------------------------------------------------------ pages
    def _rank(self, column: str) -> torch.Tensor:
        """the str column's code -> rank table on the device, made again when the dictionary has grown"""
        words = self.dictionary(column)
        cached = self._ranks.get(column)
        if cached is None or cached.numel() != max(1, len(words)):
            table = rank_table(words) if words else np.zeros((1,), dtype=np.int32)  # (no word yet: every row is NULL)
            cached = self._ranks[column] = torch.from_numpy(table).to(self.rows.device)
        return cached

    def page(self, mask: Optional[RowMask], order_by: Optional[str], ascending: bool, offset: int, limit: int,
             max_blocks: int = 0) -> Optional[np.ndarray]:
        """One page of the document listing, selected on the device: of the rows of ``mask`` (None: every present row) the offsets of
        rank ``[offset, offset + limit)`` in ``AnnLite.filter``'s order -- by the declared column ``order_by`` (rows without a value
        first ascending, last descending; equal values in ascending offset) or, without one, in ascending offset --, as i64 [<= limit].
        Only the page crosses to the host: one copy of ``limit + 1`` ints.  None where the host has to answer: ``order_by`` is not
        declared or is irregular, ``limit`` is not in ``1 .. PAGE_MAX``, ``offset`` is negative, ``offset + limit >= 2**31``, or the
        store holds no rows."""
        if self._n == 0 or type(limit) not in (int, bool) or type(offset) not in (int, bool):
            return None
        if not 1 <= limit <= PAGE_MAX or offset < 0 or offset + limit >= 2 ** 31:
            return None
        if order_by is not None and (self.kinds.get(order_by) is None or order_by in self.irregular):
            return None
        from . import ops

        if self._workspace is None:
            self._workspace = ops.ScanWorkspace()
        W = self.n_words
        words = None if mask is None else mask.words_for(W)
        out = torch.empty((limit + 1,), dtype=torch.int32, device=self.rows.device)  # (the rows, and behind them their number)
        if order_by is None:
            bits, and_bits = (self.rows, None) if words is None else (words, self.rows)
            ops.bitmap_page(bits, self._n, W, offset, limit, and_bits=and_bits, out=out, workspace=self._workspace, max_blocks=max_blocks)
        else:
            kind = self.kinds[order_by]
            ops.order_page(words, self.rows, self.values[order_by], kind, self.present[order_by], self._n, W, not ascending, offset, limit,
                           rank=self._rank(order_by) if kind == CODE else None, out=out, workspace=self._workspace, max_blocks=max_blocks)
        host = out.cpu().numpy()
        return host[: int(host[limit])].astype(np.int64)
