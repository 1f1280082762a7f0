"""Host-side mirror of lightmotif's scoring interface on top of the HIP C ABI.

Two layers, both thin:

* :class:`Pipeline` -- the reference's trait surface (``Encode`` / ``Stripe`` /
  ``Score`` / ``Maximum`` / ``Threshold``, lightmotif/src/pli/mod.rs:34-222) for the
  ``Hip`` back-end: same method names, argument meaning and error behaviour
  (misuse raises where the reference panics; degenerate input gives empty results).
* ``EncodedSequence`` / ``StripedSequence`` / ``CountMatrix`` / ``WeightMatrix`` /
  ``ScoringMatrix`` / ``StripedScores`` / ``create`` / ``stripe`` / ``scan`` -- the
  user-facing objects of the reference's Python module
  (lightmotif-py/lightmotif/lib.rs, lib.pyi) so its tests read the same here.

All sequence and score data live in device memory; every scoring operation runs
in the hand-written gfx950 kernels.  Nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from ._ffi import Coords, InvalidSymbol, LightmotifHipError, SetHit, UnsupportedBackend, check

__all__ = [
    "pack_2bit", "fasta_names",
    "Pipeline", "EncodedSequence", "StripedSequence", "StripedSequenceSet", "RegionMap", "SetHits", "SetBest", "SetCounts", "SetSums", "SetExpectedCounts", "posterior_gains", "expected_to_scoring", "SetVariantEffects", "SetVariantHits", "ScoreDistributions", "CountMatrix", "WeightMatrix",
    "background_from_counts", "markov_from_counts", "decode",
    "ScoringMatrix", "DiscreteMatrix", "StripedScores", "Scanner", "Hit", "Motif", "create", "stripe", "scan",
    "UnsupportedBackend", "InvalidSymbol", "LightmotifHipError", "DEFAULT_COLUMNS",
]

DNA_SYMBOLS = "ACTGN"                     # abc.rs:106-108
PROTEIN_SYMBOLS = "ACDEFGHIKLMNPQRSTVWYX"  # abc.rs:193-256
DEFAULT_COLUMNS = 32                      # dispatch.rs:45 / dense.rs:17 on x86-64


def _symbols(protein: bool) -> str:
    return PROTEIN_SYMBOLS if protein else DNA_SYMBOLS


def _k(protein: bool) -> int:
    return len(_symbols(protein))


def _same_alphabet(matrix, seq: "StripedSequence") -> None:
    """The reference's ``ScoringMatrix<A>`` / ``StripedSequence<A>`` share the alphabet parameter; here a mismatch is a
    ``ValueError`` before anything runs (the fused forms hand the C ABI a raw data pointer, which it cannot check)."""
    if matrix.protein != seq.protein:
        raise ValueError(f"{'protein' if matrix.protein else 'DNA'} matrix against a "
                         f"{'protein' if seq.protein else 'DNA'} sequence")


def stride(cols: int, elem_size: int) -> int:
    """DenseMatrix::stride (dense.rs:126-128)."""
    return int(_ffi.lib().lm_hip_stride(cols, elem_size))


# --- Pipeline -----------------------------------------------------------------


class _HostBlock:
    """A malloc'ed block returned by the library, exposed to numpy through the array
    interface and released with ``lm_hip_free`` when the last array on it dies."""

    def __init__(self, L, addr: int, nbytes: int):
        self._L, self._addr = L, addr
        self.__array_interface__ = {"data": (addr, False), "shape": (nbytes,), "typestr": "|u1",
                                    "version": 3}

    def __del__(self):
        try:
            self._L.lm_hip_free(C.c_void_p(self._addr))
        except Exception:  # interpreter shutdown
            pass


class Pipeline:
    """``Pipeline<A, Hip>``: owns a device context (stream + scratch)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        L = _ffi.lib()
        h = C.c_void_p()
        if stream is None:
            check(L.lm_hip_ctx_create(device, C.byref(h)))
        else:
            check(L.lm_hip_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)))
        self._L = L
        self._h = h
        self.device = device

    # Pipeline::avx2()/neon() return Result<_, UnsupportedBackend> (pli/mod.rs:401-407)
    @classmethod
    def hip(cls, device: int = 0, stream: Optional[int] = None) -> "Pipeline":
        return cls(device, stream)

    @staticmethod
    def device_count() -> int:
        n = C.c_int(0)
        check(_ffi.lib().lm_hip_device_count(C.byref(n)))
        return n.value

    @staticmethod
    def device_ordinals() -> List[int]:
        """HIP ordinals of the usable (gfx950) devices -- what ``Pipeline.hip(device)`` takes;
        on a node with other GPUs in between this is not ``range(device_count())``."""
        out, o = [], C.c_int(0)
        for i in range(Pipeline.device_count()):
            check(_ffi.lib().lm_hip_device_ordinal(i, C.byref(o)))
            out.append(o.value)
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.lm_hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self) -> None:
        check(self._L.lm_hip_ctx_sync(self._h))

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        check(self._L.lm_hip_ctx_stream(self._h, C.byref(s)))
        return s.value or 0

    def set_rows_per_stream(self, rows: int) -> None:
        check(self._L.lm_hip_ctx_set_rows_per_stream(self._h, rows))

    def set_prefilter(self, enabled: bool) -> None:
        check(self._L.lm_hip_ctx_set_prefilter(self._h, int(enabled)))

    def set_track_argmax(self, enabled: bool) -> None:
        """``score_into`` on large matrices also tracks the maximum so that ``argmax`` on the
        same scores is free (default on)."""
        check(self._L.lm_hip_ctx_set_track_argmax(self._h, int(enabled)))

    def set_option(self, name: str, value: float) -> None:
        """An alternative path inside the library with identical results (``lm_hip_ctx_set_option``): for tests and A/B runs."""
        check(self._L.lm_hip_ctx_set_option(self._h, name.encode(), float(value)))

    @property
    def last_kernel(self) -> str:
        return self._L.lm_hip_ctx_last_kernel(self._h).decode()

    @property
    def last_stream_rows(self) -> int:
        """Rows per stream T of the last plain store launch (``score_into`` without the tracked maximum) when one C = 32
        store kernel carried it; 0 when it took another route (lm_hip_ctx_last_stream_rows)."""
        return int(self._L.lm_hip_ctx_last_stream_rows(self._h))

    @staticmethod
    def _registry_rows(call) -> Dict[Tuple[str, int, int, str], int]:
        n = C.c_size_t(0)
        check(call(None, 0, C.byref(n)))
        rows = (_ffi.RegistryRow * max(n.value, 1))()
        check(call(rows, n.value, C.byref(n)))
        return {(_ffi.FAMILIES[r.family], r.wide, r.m, _ffi.SLOTS[r.slot] if r.family == 0 else ""): int(r.value)
                for r in rows[:n.value]}

    @staticmethod
    def registry_rows() -> Dict[Tuple[str, int, int, str], int]:
        """Every kernel row the build registered, ``(family, wide, M, slot) -> id`` (lm_hip_registry_rows): rows with
        equal ids share one kernel; ``slot`` is "" outside the "c32" family.  Needs no device."""
        return Pipeline._registry_rows(_ffi.lib().lm_hip_registry_rows)

    def launch_tally(self) -> Dict[Tuple[str, int, int, str], int]:
        """With ``set_option("tally_launches", 1)``: the registry rows this pipeline launched since the last call,
        ``(family, wide, M, slot) -> launches``; reading clears the tally (lm_hip_ctx_launch_tally)."""
        return Pipeline._registry_rows(lambda rows, cap, n: self._L.lm_hip_ctx_launch_tally(self._h, rows, cap, n))

    @property
    def last_scan_counts(self) -> Tuple[int, int]:
        """(hits, candidate pieces) of the last fused threshold scan on this pipeline (lm_hip_ctx_last_scan_counts)."""
        h, c = C.c_ulonglong(0), C.c_ulonglong(0)
        check(self._L.lm_hip_ctx_last_scan_counts(self._h, C.byref(h), C.byref(c)))
        return int(h.value), int(c.value)

    @property
    def last_phases_ms(self) -> Optional[Tuple[float, float, float, float]]:
        """(scan, re-scoring, ordering, host share) of the last fused threshold call in ms, with ``set_option("time_scan", 1)``;
        None otherwise (lm_hip_ctx_last_phases_ms)."""
        ph = (C.c_float * 4)()
        check(self._L.lm_hip_ctx_last_phases_ms(self._h, ph))
        return tuple(float(x) for x in ph) if ph[0] >= 0 else None

    @property
    def last_scan_info(self) -> Tuple[int, int]:
        """(motif rows scanned, LDS table bytes per position) of the last single-job fused scan on this pipeline; zeros
        when no prefilter / exact scan kernel ran (lm_hip_ctx_last_scan_info)."""
        r, b = C.c_size_t(0), C.c_size_t(0)
        check(self._L.lm_hip_ctx_last_scan_info(self._h, C.byref(r), C.byref(b)))
        return int(r.value), int(b.value)

    @property
    def last_scan_kernel_ms(self) -> Optional[float]:
        """Duration of the scan kernel(s) of the last fused call, with ``set_option("time_scan", 1)``; None otherwise
        (lm_hip_ctx_last_scan_kernel_ms)."""
        ms = C.c_float(-1.0)
        check(self._L.lm_hip_ctx_last_scan_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value) if ms.value >= 0 else None

    def sustained_clock_mhz(self, load, seconds: float = 0.25, window_us: int = 3000):
        """Shader clock (MHz, median over windows) the device sustains while `load()` is called back to back for
        `seconds` from this thread; a second thread runs lm_hip_device_clock_mhz windows beside it.  Returns
        (mhz or None, ms per call with the probe running, ms per call without)."""
        import threading
        import time
        dev = C.c_int(self.device)

        def run(duration):
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < duration:
                load()
                n += 1
            self.sync()
            return (time.perf_counter() - t0) / max(n, 1) * 1e3
        run(0.05)
        alone = run(seconds / 2)
        samples, stop = [], threading.Event()

        def sampler():
            mhz = C.c_double(0.0)
            while not stop.is_set():
                if self._L.lm_hip_device_clock_mhz(dev.value, window_us, C.byref(mhz)) == 0:
                    samples.append(mhz.value)
        th = threading.Thread(target=sampler)
        th.start()
        beside = run(seconds)
        stop.set()
        th.join()
        s = sorted(samples[1:-1] if len(samples) > 4 else samples)
        return (s[len(s) // 2] if s else None), beside, alone

    # -- Encode / Stripe (pli/mod.rs:34-67, 164-201) ---------------------------

    def encode(self, sequence: Union[str, bytes], protein: bool = False) -> "EncodedSequence":
        return EncodedSequence(sequence, protein=protein)

    def stripe(self, encoded: "EncodedSequence", columns: int = DEFAULT_COLUMNS) -> "StripedSequence":
        h = C.c_void_p()
        data = np.ascontiguousarray(encoded.data, dtype=np.uint8)
        check(self._L.lm_hip_seq_from_encoded(self._h, data.ctypes.data, data.size, columns,
                                              _k(encoded.protein), C.byref(h)))
        return StripedSequence(self, h, encoded.protein)

    def stripe_2bit(self, packed: np.ndarray, length: int, n_mask: Optional[np.ndarray] = None,
                    columns: int = DEFAULT_COLUMNS, n_runs: Optional[np.ndarray] = None) -> "StripedSequence":
        """A DNA sequence held 4 bases per byte (``pack_2bit``) -> resident StripedSequence: a quarter of the
        bytes over PCIe, unpacked straight into the striped matrix (``lm_hip_seq_from_2bit``).  N positions as an
        ``(n, 2)`` array of runs ``(start, size)`` -- the .2bit container's form -- and / or as a bit mask."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        if packed.size < (length + 3) // 4:
            raise ValueError("packed buffer shorter than length / 4")
        mptr = rptr = None
        nruns = 0
        if n_mask is not None:
            n_mask = np.ascontiguousarray(n_mask, dtype=np.uint8)
            if n_mask.size < (length + 7) // 8:
                raise ValueError("N mask shorter than length / 8")
            mptr = n_mask.ctypes.data
        if n_runs is not None and len(n_runs):
            n_runs = np.ascontiguousarray(np.asarray(n_runs, dtype=np.uint64).reshape(-1, 2))
            rptr, nruns = n_runs.ctypes.data, n_runs.shape[0]
        h = C.c_void_p()
        check(self._L.lm_hip_seq_from_2bit(self._h, packed.ctypes.data, mptr, rptr, nruns, length, columns, C.byref(h)))
        return StripedSequence(self, h, False)

    def stripe_ascii(self, sequence: Union[str, bytes, np.ndarray], protein: bool = False, lossy: bool = False,
                     columns: int = DEFAULT_COLUMNS) -> "StripedSequence":
        """encode (+ encode_lossy) and stripe entirely on the device."""
        if isinstance(sequence, np.ndarray):     # a genome already in memory as bytes: no copy
            raw = buf = np.ascontiguousarray(sequence, dtype=np.uint8)
        else:
            raw = sequence.encode("ascii", "replace") if isinstance(sequence, str) else bytes(sequence)
            buf = np.frombuffer(raw, dtype=np.uint8)
        h = C.c_void_p()
        bad = C.c_size_t(0)
        st = self._L.lm_hip_seq_from_ascii(self._h, b"P" if protein else b"D", buf.ctypes.data,
                                           buf.size, columns, int(lossy), C.byref(h), C.byref(bad))
        if st == _ffi.ERR_INVALID_SYMBOL:
            raise InvalidSymbol(f"Invalid symbol in sequence: {chr(int(raw[bad.value]))!r}")
        check(st)
        return StripedSequence(self, h, protein)

    def stripe_ascii_set(self, records: Sequence[Union[str, bytes, np.ndarray]], protein: bool = False, lossy: bool = False,
                         columns: int = DEFAULT_COLUMNS, offsets: Optional[np.ndarray] = None) -> "StripedSequenceSet":
        """Many records -> ONE resident striped sequence (their texts joined, no separators) plus the table of record
        offsets: one upload, encode + stripe on the device (``lm_hip_seqset_from_ascii``).  ``records`` is a list of texts,
        or ONE uint8 array holding the joined text together with ``offsets`` (``n + 1`` ascending positions, first 0)."""
        if offsets is not None:
            buf = np.ascontiguousarray(records, dtype=np.uint8)
            offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        else:
            raws = [r.tobytes() if isinstance(r, np.ndarray) else r.encode("ascii", "replace") if isinstance(r, str) else bytes(r)
                    for r in records]
            offs = np.zeros(len(raws) + 1, dtype=np.uint64)
            np.cumsum([len(r) for r in raws], out=offs[1:])
            buf = np.frombuffer(b"".join(raws), dtype=np.uint8)
        if offs.ndim != 1 or offs.size == 0:
            raise ValueError("offsets: one entry per record and one more")
        h = C.c_void_p()
        bad_r, bad_i = C.c_size_t(0), C.c_size_t(0)
        st = self._L.lm_hip_seqset_from_ascii(self._h, b"P" if protein else b"D", buf.ctypes.data if buf.size else None, buf.size,
                                              offs.ctypes.data, offs.size - 1, columns, int(lossy), C.byref(h), C.byref(bad_r),
                                              C.byref(bad_i))
        if st == _ffi.ERR_INVALID_SYMBOL:
            byte = int(buf[int(offs[bad_r.value]) + bad_i.value])
            raise InvalidSymbol(f"Invalid symbol in sequence {bad_r.value} at position {bad_i.value}: {chr(byte)!r}")
        check(st)
        return StripedSequenceSet(self, h, protein)

    def stripe_fasta_set(self, data, protein: bool = False, lossy: bool = False,
                         columns: int = DEFAULT_COLUMNS) -> "StripedSequenceSet":
        """The bytes of a FASTA file -> ONE resident striped sequence of its records, parsed on the device
        (``lm_hip_seqset_from_fasta``; the grammar is stated there): the host uploads ``data`` -- ``bytes``, ``bytearray``,
        ``memoryview`` or a uint8 array, passed without a copy -- and never looks at a sequence line.  The set equals
        ``stripe_ascii_set`` of the parsed records and carries ``header_spans``: per record the bytes ``[begin, end)`` of
        ``data`` that hold its header line (``fasta_names(data, spans)`` gives the names)."""
        buf = np.ascontiguousarray(data, dtype=np.uint8) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        h, spans = C.c_void_p(), C.c_void_p()
        n, bad_r, bad_i = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        st = self._L.lm_hip_seqset_from_fasta(self._h, b"P" if protein else b"D", buf.ctypes.data if buf.size else None, buf.size,
                                              columns, int(lossy), C.byref(h), C.byref(spans), C.byref(n), C.byref(bad_r),
                                              C.byref(bad_i))
        if st == _ffi.ERR_INVALID_SYMBOL:
            err = InvalidSymbol(f"Invalid symbol in sequence {bad_r.value} at position {bad_i.value}")
            err.record, err.index = bad_r.value, bad_i.value
            raise err
        check(st)
        out = StripedSequenceSet(self, h, protein)
        out.header_spans = self._take_array(spans, 2 * n.value, np.uint64).reshape(n.value, 2)
        return out

    def stripe_set(self, encoded: Sequence["EncodedSequence"], columns: int = DEFAULT_COLUMNS,
                   protein: Optional[bool] = None) -> "StripedSequenceSet":
        """The same from already encoded records (``lm_hip_seqset_from_encoded``).  ``protein`` names the alphabet of a set
        without records (DNA when left out); with records it must be theirs."""
        alphabets = {e.protein for e in encoded} | ({bool(protein)} if protein is not None else set())
        if len(alphabets) > 1:
            raise ValueError("the records of a set share one alphabet")
        protein = bool(alphabets.pop()) if alphabets else False
        parts = [np.ascontiguousarray(e.data, dtype=np.uint8) for e in encoded]
        offs = np.zeros(len(parts) + 1, dtype=np.uint64)
        np.cumsum([p.size for p in parts], out=offs[1:])
        buf = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        h = C.c_void_p()
        check(self._L.lm_hip_seqset_from_encoded(self._h, buf.ctypes.data if buf.size else None, buf.size, offs.ctypes.data,
                                                 offs.size - 1, columns, _k(protein), C.byref(h)))
        return StripedSequenceSet(self, h, protein)

    def sample_set(self, lengths, background, transitions=None, *, seed: int = 0, record_base: int = 0, protein: bool = False,
                   columns: int = DEFAULT_COLUMNS) -> "StripedSequenceSet":
        """A null set drawn on the device (``lm_hip_seqset_sample``; seq.rs:131-143, seq.rs:315-328 for every record at once):
        record ``r`` holds ``lengths[r]`` symbols drawn from ``background`` -- ``k`` f32 frequencies for all records, or a
        ``(records, k)`` table with one row per record -- or, with ``transitions`` (``(k, k)``, DNA only, one model per call),
        from the first-order chain that starts in ``background``.  A record's text depends on ``seed``, on its number
        ``record_base + r`` and on its model alone; the header spells out the rule, which a numpy restatement reproduces bit
        for bit."""
        k = _k(protein)
        n = _u64_array(lengths)
        f = np.ascontiguousarray(background, dtype=np.float32)
        if f.ndim not in (1, 2) or f.shape[-1] != k:
            raise ValueError(f"background: {k} frequencies, or a (records, {k}) table")
        if f.ndim == 2 and f.shape[0] != n.size:
            raise ValueError(f"{f.shape[0]} models for {n.size} records")
        t = None
        if transitions is not None:
            t = np.ascontiguousarray(transitions, dtype=np.float32)
            if t.shape != (k, k):
                raise ValueError(f"transitions: a ({k}, {k}) table")
        h = C.c_void_p()
        check(self._L.lm_hip_seqset_sample(self._h, b"P" if protein else b"D", _ptr(n), n.size, _ptr(f), 1 if f.ndim == 1 else n.size,
                                           t.ctypes.data if t is not None else None, int(seed) % (1 << 64),
                                           int(record_base) % (1 << 64), columns, C.byref(h)))
        return StripedSequenceSet(self, h, protein)

    def scan_threshold_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], thresholds: Optional[Sequence[float]],
                           seqset: "StripedSequenceSet") -> "SetHits":
        """``n`` motifs x every record of the set in one call (the CLI's whole job product, main.rs:502-561).  Per motif:
        ``(records int64, positions int64, scores f32)`` with ``score >= t`` and ``position + M <= len(record)``
        (scan.rs:185-190), ascending in (record, position) -- views cut from one block the library returned."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms, thresholds)
        if batch.protein - {seqset.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seqset.protein), seqset)
        n = len(batch)
        counts = np.zeros(n, dtype=np.uintp)
        ptr = C.POINTER(SetHit)()
        check(self._L.lm_hip_scan_threshold_seqset(self._h, batch.handles, batch.thresholds, n, seqset._h,
                                                   counts.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(ptr)))
        total = int(counts.sum())
        raw = self._take_array(ptr, total * C.sizeof(SetHit), np.uint8)
        return SetHits(raw.view(SET_HIT_DTYPE) if total else np.zeros(0, dtype=SET_HIT_DTYPE), counts)

    def scan_best_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], seqset: "StripedSequenceSet") -> "SetBest":
        """The dense ``motifs x records`` matrix of best windows in one call (``lm_hip_scan_best_seqset``): per (motif,
        record) the greatest score over the windows ``position + M <= len(record)`` (scan.rs:185-190) and the LOWEST
        position holding it; NaN windows never compete.  No score matrix and no hit list exist on the way."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms)
        if batch.protein - {seqset.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seqset.protein), seqset)
        n, records = len(batch), len(seqset)
        raw = np.zeros(n * records, dtype=SET_BEST_DTYPE)
        check(self._L.lm_hip_scan_best_seqset(self._h, batch.handles, n, seqset._h,
                                              raw.ctypes.data_as(C.POINTER(_ffi.SetBest)) if raw.size else None))
        return SetBest(raw.reshape(n, records), self.last_kernel if raw.size else "")

    def scan_count_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], thresholds,
                       seqset: "StripedSequenceSet") -> "SetCounts":
        """How many windows of every motif reach its cut-offs in every record, in one call and without a hit list
        (``lm_hip_scan_count_seqset``).  ``thresholds`` has shape ``(n,)`` or ``(n, levels)``, ``1 <= levels <= 4``: several
        cut-offs of a motif cost one walk.  A window ``position + M <= len(record)`` (scan.rs:185-190) counts at a level
        when ``score >= t`` in f32; NaN windows and NaN thresholds count nothing.  Of a ``MotifBatch`` only the handles are
        used."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms)
        if batch.protein - {seqset.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seqset.protein), seqset)
        n, records = len(batch), len(seqset)
        ts = np.ascontiguousarray(thresholds, dtype=np.float32)
        if ts.ndim == 1:
            ts = ts.reshape(-1, 1)
        if ts.ndim != 2 or ts.shape[0] != n:
            raise ValueError("thresholds: one per motif, or one row of cut-offs per motif")
        levels = ts.shape[1]
        if not 1 <= levels <= _ffi.MAX_COUNT_LEVELS:
            raise ValueError(f"{levels} cut-offs per motif: a call takes 1 ... {_ffi.MAX_COUNT_LEVELS}")
        counts = np.zeros((n, levels, records), dtype=np.uint32)
        check(self._L.lm_hip_scan_count_seqset(self._h, batch.handles, ts.ctypes.data_as(C.POINTER(C.c_float)), levels, n, seqset._h,
                                               counts.ctypes.data_as(C.POINTER(C.c_uint32)) if counts.size else None))
        lengths = seqset.lengths.reshape(1, -1)
        rows = np.asarray([len(p) for p in batch.pssms], dtype=np.int64).reshape(-1, 1)
        return SetCounts(counts, np.maximum(0, lengths - rows + 1), self.last_kernel if counts.size else "")

    def scan_sum_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], seqset: "StripedSequenceSet", scale=None) -> "SetSums":
        """The total odds of every motif in every record, in one call and without a hit list (``lm_hip_scan_sum_seqset``):
        per (motif, record) the f64 sum of ``2 ** (scale * score)`` over the windows ``position + M <= len(record)``
        (scan.rs:185-190); NaN windows add nothing.  ``scale`` is None (1: log2-odds matrices), one number or one per motif,
        finite and > 0 (``log2(base)`` for a matrix in another base, or a temperature).  Of a ``MotifBatch`` only the
        handles are used."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms)
        if batch.protein - {seqset.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seqset.protein), seqset)
        n, records = len(batch), len(seqset)
        scales = None
        if scale is not None:
            scales = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float32), (n,)) if np.ndim(scale) == 0 else scale,
                                          dtype=np.float32)
            if scales.shape != (n,):
                raise ValueError("scale: one number, or one per motif")
        sums = np.zeros((n, records), dtype=np.float64)
        check(self._L.lm_hip_scan_sum_seqset(self._h, batch.handles, scales.ctypes.data_as(C.POINTER(C.c_float)) if scales is not None else None,
                                             n, seqset._h, sums.ctypes.data_as(C.POINTER(C.c_double)) if sums.size else None))
        lengths = seqset.lengths.reshape(1, -1)
        rows = np.asarray([len(p) for p in batch.pssms], dtype=np.int64).reshape(-1, 1)
        return SetSums(sums, np.maximum(0, lengths - rows + 1), self.last_kernel if sums.size else "")

    def expected_counts_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], seqset: "StripedSequenceSet", gains,
                            scale=None) -> "SetExpectedCounts":
        """The expected site counts of every motif over the set in one call (``lm_hip_seqset_expected_counts``), the E-step
        of motif EM: per motif the ``(M, K)`` table ``E[j][s] = sum of z over the windows whose symbol at offset j is s``,
        ``z = min(2 ** (scale * score) * gains[motif, record], 1)`` quantised to ``2 ** -frac_bits``.  ``gains`` is
        ``(motifs, records)`` float64, finite and >= 0 (``posterior_gains`` of ``scan_sum_set``); ``scale`` as for
        ``scan_sum_set``.  The tables are a pure function of the inputs: integer sums on the device, no order."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms)
        if batch.protein - {seqset.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seqset.protein), seqset)
        n, records, k = len(batch), len(seqset), _k(seqset.protein)
        scales = None
        if scale is not None:
            scales = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float32), (n,)) if np.ndim(scale) == 0 else scale,
                                          dtype=np.float32)
            if scales.shape != (n,):
                raise ValueError("scale: one number, or one per motif")
        g = np.ascontiguousarray(gains, dtype=np.float64)
        if g.shape != (n, records):
            raise ValueError(f"gains: a ({n}, {records}) table, one gain per motif and record")
        rows = [len(p) for p in batch.pssms]
        flat = np.zeros(sum(rows) * k, dtype=np.float64)
        frac = C.c_int(0)
        check(self._L.lm_hip_seqset_expected_counts(self._h, batch.handles, scales.ctypes.data_as(C.POINTER(C.c_float)) if scales is not None else None,
                                                    g.ctypes.data_as(C.POINTER(C.c_double)) if g.size else None, n, seqset._h,
                                                    flat.ctypes.data_as(C.POINTER(C.c_double)) if flat.size else None, C.byref(frac)))
        cuts = np.cumsum([0] + [m * k for m in rows])
        tables = [flat[cuts[i]:cuts[i + 1]].reshape(rows[i], k) for i in range(n)]
        return SetExpectedCounts(tables, int(frac.value), self.last_kernel if n and records else "")

    def em_step(self, pssms: Sequence["ScoringMatrix"], seqset: "StripedSequenceSet", model: str = "oops", gamma=None, scale=None,
                pseudocount: Union[None, float, Dict[str, float]] = 0.1, background=None):
        """One iteration of motif EM on the resident set: ``scan_sum_set`` (Z per record), ``posterior_gains``,
        ``expected_counts_set`` (the E-step) and ``expected_to_scoring`` (the M-step, the f32 arithmetic of
        ``CountMatrix.to_scoring``).  Returns ``(matrices, expected, gamma, log2_likelihood)``: the new ``ScoringMatrix``
        objects, the ``SetExpectedCounts``, for ZOOPS the new ``gamma`` per motif (the mean posterior mass per record
        with a window; None for OOPS) and the log2-likelihood ratio of the matrices that came IN, per motif: the sum over
        the records with a window of ``log2 Z_r`` (OOPS) or ``log2((1 - gamma) + lambda_r Z_r)`` (ZOOPS).  ``background``
        defaults to the set's own (``seqset.background()``)."""
        pssms = list(pssms)
        sums = self.scan_sum_set(pssms, seqset, scale)
        gains = posterior_gains(sums, model, gamma)
        expected = self.expected_counts_set(pssms, seqset, gains, scale)
        bg = seqset.background() if background is None else background
        new = [expected_to_scoring(c, pseudocount, bg, protein=seqset.protein) for c in expected.counts]
        ll, new_gamma = _em_likelihood(sums, gains, model, gamma)
        return new, expected, new_gamma, ll

    def refine(self, pssms: Sequence["ScoringMatrix"], seqset: "StripedSequenceSet", iterations: int, model: str = "oops", gamma=None,
               scale=None, pseudocount: Union[None, float, Dict[str, float]] = 0.1, background=None, return_counts: bool = False):
        """``iterations`` calls of ``em_step``, each on the matrices of the one before.  Returns ``(matrices,
        log2_likelihood)``: the refined matrices and an ``(iterations + 1, motifs)`` float64 table, row ``t`` the
        log2-likelihood of the matrices after ``t`` iterations (row 0: as given), which EM does not let decrease beyond the
        fixed point's quantisation.  For ZOOPS ``gamma`` (default 0.5) is re-estimated at every iteration.  With
        ``return_counts`` a third value follows: the ``SetExpectedCounts`` of the last iteration (None without one)."""
        mats = list(pssms)
        if model == "zoops" and gamma is None:
            gamma = 0.5
        bg = seqset.background() if background is None else background
        lls, expected = [], None
        for _ in range(int(iterations)):
            mats, expected, new_gamma, ll = self.em_step(mats, seqset, model, gamma, scale, pseudocount, bg)
            lls.append(ll)
            if new_gamma is not None:
                gamma = np.clip(new_gamma, 1e-6, 1.0)
        sums = self.scan_sum_set(mats, seqset, scale)
        lls.append(_em_likelihood(sums, posterior_gains(sums, model, gamma), model, gamma)[0])
        lls = np.asarray(lls, dtype=np.float64)
        return (mats, lls, expected) if return_counts else (mats, lls)

    def _variant_args(self, batch: "MotifBatch", seqset: "StripedSequenceSet", records, positions, alts) -> np.ndarray:
        """The ``lm_hip_variant`` list of a call: records and positions as ``_u64_array`` takes them, ``alts`` symbol indices
        or a str / bytes of letters (strict table: an unknown letter raises)."""
        if batch.protein - {seqset.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seqset.protein), seqset)
        rec, pos = _u64_array(records), _u64_array(positions)
        if isinstance(alts, (str, bytes, bytearray)):
            raw = np.frombuffer(alts.encode("latin-1") if isinstance(alts, str) else bytes(alts), dtype=np.uint8)
            table = np.full(256, 255, dtype=np.uint8)
            table[np.frombuffer(_symbols(seqset.protein).encode(), dtype=np.uint8)] = np.arange(_k(seqset.protein), dtype=np.uint8)
            alt = table[raw]
            if (alt == 255).any():
                raise InvalidSymbol(f"Invalid symbol: {chr(int(raw[int(np.argmax(alt == 255))]))!r}")
        else:
            a = np.asarray(alts)
            if a.size and a.dtype.kind not in "iu":
                raise TypeError("alts are symbol indices or letters")
            alt = np.where((a < 0) | (a > 255), 255, a).astype(np.uint8) if a.size else np.zeros(0, np.uint8)
        if not rec.shape == pos.shape == alt.shape:
            raise ValueError(f"{rec.size} records, {pos.size} positions and {alt.size} alts")
        out = np.zeros(rec.size, dtype=VARIANT_DTYPE)
        out["record"], out["position"], out["alt"] = rec, pos, alt
        return out

    def scan_variants_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], seqset: "StripedSequenceSet",
                          records, positions, alts) -> "SetVariantEffects":
        """What each single-symbol substitution ``(record, position, alt)`` does to the best window of every motif that
        covers it (``lm_hip_seqset_variant_effects``): the dense ``(motifs, variants)`` block of both alleles' best scores
        and window starts.  Windows lie inside the record; NaN windows never compete, the lowest start wins a tie.  An
        invalid variant (no such record, a position outside it, no such symbol) is not an error: every motif reports
        none for it."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms)
        v = self._variant_args(batch, seqset, records, positions, alts)
        n = len(batch)
        raw = np.zeros((n, v.size), dtype=VARIANT_EFFECT_DTYPE)
        ref = np.full(v.size, 255, dtype=np.uint8)
        spare = np.zeros(2, dtype=np.uint64)      # (an empty block still has to be a pointer)
        check(self._L.lm_hip_seqset_variant_effects(self._h, batch.handles, n, seqset._h, v.ctypes.data if v.size else None, v.size,
                                                    raw.ctypes.data if raw.size else spare.ctypes.data,
                                                    ref.ctypes.data if ref.size else None))
        if n == 0 and v.size:       # (nothing ran: the resident symbols come from a call of their own)
            return SetVariantEffects(raw, v, self._variant_symbols(seqset, v), "")
        return SetVariantEffects(raw, v, ref, self.last_kernel if raw.size else "")

    def _variant_symbols(self, seqset: "StripedSequenceSet", v: np.ndarray) -> np.ndarray:
        """The resident symbol of every variant, 255 where it is invalid."""
        k = _k(seqset.protein)
        sym, ok = seqset._windows(np.array([v.size], dtype=np.uintp), np.array([1], dtype=np.uintp), np.zeros(1, dtype=np.int64),
                                  np.ascontiguousarray(np.stack([v["record"], v["position"]], axis=1)), 16)
        return np.where((ok != 0) & (v["alt"] < k), sym, 255).astype(np.uint8)

    def scan_variant_hits_set(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"], thresholds: Optional[Sequence[float]],
                              seqset: "StripedSequenceSet", records, positions, alts) -> "SetVariantHits":
        """The sparse form of ``scan_variants_set`` (``lm_hip_seqset_variant_hits``): per motif the (variant, effect) pairs
        with ``ref_score >= t`` or ``alt_score >= t``, ascending in the variant's index; the dense block never leaves the
        device.  ``thresholds=None`` takes the batch's."""
        batch = pssms if isinstance(pssms, MotifBatch) and thresholds is None else \
            MotifBatch(self, pssms.pssms if isinstance(pssms, MotifBatch) else pssms, thresholds)
        if len(batch) and batch.thresholds is None:
            raise ValueError("no thresholds: pass them, or a batch prepared with them")
        v = self._variant_args(batch, seqset, records, positions, alts)
        n = len(batch)
        counts = np.zeros(n, dtype=np.uintp)
        ref = np.full(v.size, 255, dtype=np.uint8)
        ptr = C.c_void_p()
        check(self._L.lm_hip_seqset_variant_hits(self._h, batch.handles, batch.thresholds, n, seqset._h, v.ctypes.data if v.size else None,
                                                 v.size, counts.ctypes.data if n else None, C.byref(ptr), ref.ctypes.data if ref.size else None))
        total = int(counts.sum())
        raw = self._take_array(ptr, total * VARIANT_HIT_DTYPE.itemsize, np.uint8)
        if n == 0 and v.size:
            ref = self._variant_symbols(seqset, v)
        return SetVariantHits(raw.view(VARIANT_HIT_DTYPE) if total else np.zeros(0, dtype=VARIANT_HIT_DTYPE), counts, v, ref,
                              self.last_kernel if n and v.size else "")

    def score_distributions(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"]) -> "ScoreDistributions":
        """The score distributions (pwm/dist.rs:51-226) of a whole motif list, built and kept on the device
        (``lm_hip_dists_create``): one call instead of one ``ScoringMatrix.score_distribution`` per motif, bit-identical
        to it.  Holds ``8 * (1000 * sum(M) + n)`` bytes of device memory."""
        return ScoreDistributions(self, pssms.pssms if isinstance(pssms, MotifBatch) else pssms)

    def upload(self, data: np.ndarray, length: int, wrap: int, columns: int,
               protein: bool = False) -> "StripedSequence":
        """Adopt an already striped host matrix ((rows+wrap) x stride u8)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        h = C.c_void_p()
        check(self._L.lm_hip_seq_upload(self._h, data.ctypes.data, data.shape[0], data.shape[1],
                                        columns, wrap, length, _k(protein), C.byref(h)))
        return StripedSequence(self, h, protein)

    def adopt_sequence(self, data_ptr: int, rows: int, wrap: int, columns: int, stride_: int,
                       length: int, protein: bool = False, keepalive=None,
                       capacity_rows: Optional[int] = None) -> "StripedSequence":
        """A StripedSequence over a striped matrix that already lives on the device and stays
        the caller's (``(rows + wrap) x stride`` bytes at ``data_ptr``, e.g. a torch tensor or
        one row shard of a multi-GPU job): nothing is copied.  ``capacity_rows`` = rows the
        buffer has room for (configure_wrap may grow into them).  ``keepalive`` is held by the
        returned object so the buffer outlives it."""
        h = C.c_void_p()
        check(self._L.lm_hip_seq_adopt_dptr(self._h, C.c_void_p(data_ptr), rows + wrap,
                                            max(capacity_rows or 0, rows + wrap), stride_, columns,
                                            wrap, length, _k(protein), C.byref(h)))
        seq = StripedSequence(self, h, protein)
        seq._keepalive = keepalive
        return seq

    # -- Score (pli/mod.rs:69-130) ----------------------------------------------

    def score_rows_into(self, pssm: "ScoringMatrix", seq: "StripedSequence", rows: range,
                        scores: "StripedScores") -> None:
        _same_alphabet(pssm, seq)
        check(self._L.lm_hip_score_rows_into(self._h, pssm._device(self), seq._h,
                                             rows.start, max(rows.stop, rows.start), scores._h))

    def score_into(self, pssm: "ScoringMatrix", seq: "StripedSequence",
                   scores: "StripedScores") -> None:
        _same_alphabet(pssm, seq)
        check(self._L.lm_hip_score_into(self._h, pssm._device(self), seq._h, scores._h))

    def score(self, pssm: "ScoringMatrix", seq: "StripedSequence") -> "StripedScores":
        scores = StripedScores.empty(self, seq.columns)
        self.score_into(pssm, seq, scores)
        return scores

    # -- Maximum / Threshold (pli/mod.rs:132-161, 203-222) ------------------------

    def argmax(self, scores: "StripedScores") -> Optional[Tuple[int, int]]:
        found, best, _ = self._argmax(scores)
        return (best.row, best.col) if found else None

    def max(self, scores: "StripedScores") -> Optional[float]:
        """``Maximum::max`` (pli/mod.rs:158-160) through its own export, ``lm_hip_max``."""
        found, value = C.c_int(0), C.c_float(0)
        check(self._L.lm_hip_max(self._h, scores._h, C.byref(found), C.byref(value)))
        return float(value.value) if found.value else None

    def _argmax(self, scores: "StripedScores"):
        found, best, value = C.c_int(0), Coords(), C.c_float(0)
        check(self._L.lm_hip_argmax(self._h, scores._h, C.byref(found), C.byref(best), C.byref(value)))
        return bool(found.value), best, float(value.value)

    def argmax_handle_shard(self, scores: "StripedScores", first_cell_rule: bool):
        """``((row, col), value)`` of one row shard held in a handle (rows relative to the
        shard), with the first-cell rule applied only when the shard holds row 0."""
        scores.set_first_cell_rule(first_cell_rule)
        found, best, value = self._argmax(scores)
        return ((best.row, best.col), value) if found else None

    def threshold(self, scores: "StripedScores", threshold: float) -> List[Tuple[int, int]]:
        ptr, n = C.POINTER(Coords)(), C.c_size_t(0)
        check(self._L.lm_hip_threshold(self._h, scores._h, threshold, C.byref(ptr), C.byref(n)))
        return self._take_coords(ptr, n.value)

    def _take_coords(self, ptr, n: int) -> List[Tuple[int, int]]:
        try:
            if n == 0:
                return []
            arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_size_t)), shape=(n, 2))
            return [(int(r), int(c)) for r, c in arr]
        finally:
            if ptr:
                self._L.lm_hip_free(ptr)

    # -- fused forms ----------------------------------------------------------------

    def score_argmax(self, pssm: "ScoringMatrix", seq: "StripedSequence",
                     rows: Optional[range] = None):
        """score_rows_into + argmax without writing the scores: ((row, col), value) or None."""
        _same_alphabet(pssm, seq)
        length, wrap, nrows, stride_, columns, data_ptr = seq._info()    # one call: a small scan is latency-bound
        rows = range(0, nrows) if rows is None else rows
        found, best, value = C.c_int(0), Coords(), C.c_float(0)
        check(self._L.lm_hip_score_argmax_f32_dptr(
            self._h, pssm._device(self), data_ptr, nrows + wrap, stride_, columns,
            wrap, length, rows.start, max(rows.stop, rows.start), C.byref(found),
            C.byref(best), C.byref(value)))
        return ((best.row, best.col), float(value.value)) if found.value else None

    def score_threshold(self, pssm: "ScoringMatrix", seq: "StripedSequence", threshold: float,
                        rows: Optional[range] = None):
        """score_rows_into + threshold without writing the scores: ([(row, col)], [value])."""
        _same_alphabet(pssm, seq)
        length, wrap, nrows, stride_, columns, data_ptr = seq._info()
        rows = range(0, nrows) if rows is None else rows
        ptr, vals, n = C.POINTER(Coords)(), C.POINTER(C.c_float)(), C.c_size_t(0)
        check(self._L.lm_hip_score_threshold_f32_dptr(
            self._h, pssm._device(self), data_ptr, nrows + wrap, stride_, columns,
            wrap, length, rows.start, max(rows.stop, rows.start), threshold,
            C.byref(ptr), C.byref(vals), C.byref(n)))
        try:
            values = [float(vals[i]) for i in range(n.value)]
        finally:
            if vals:
                self._L.lm_hip_free(vals)
        return self._take_coords(ptr, n.value), values

    # -- many motifs x one resident sequence (the CLI's job fan-out, main.rs:554-561) ----

    def scan_argmax_batch(self, pssms: Sequence["ScoringMatrix"], seq: "StripedSequence"):
        """Per motif: ``((row, col), value)`` of the best cell, or ``None`` (L < M)."""
        if any(p.protein != seq.protein for p in pssms):
            _same_alphabet(next(p for p in pssms if p.protein != seq.protein), seq)
        n = len(pssms)
        handles = (C.c_void_p * n)(*[p._device(self) for p in pssms])
        found = (C.c_int * n)()
        best = (Coords * n)()
        value = (C.c_float * n)()
        check(self._L.lm_hip_scan_argmax_batch(self._h, handles, n, seq._h, found, best, value))
        return [((best[i].row, best[i].col), float(value[i])) if found[i] else None for i in range(n)]

    def prepare_batch(self, pssms: Sequence["ScoringMatrix"], thresholds: Optional[Sequence[float]] = None) -> "MotifBatch":
        """The motif list of a batch in the form the C ABI takes it (device handles, thresholds), built once: a job loop that
        scans sequence after sequence with the same motifs (the CLI, main.rs:502-561) does not rebuild it per call."""
        return MotifBatch(self, pssms, thresholds)

    def scan_threshold_batch(self, pssms: Union[Sequence["ScoringMatrix"], "MotifBatch"],
                             thresholds: Optional[Sequence[float]], seq: "StripedSequence") -> "BatchHits":
        """Per motif: ``(coords (n_i, 2) int64 in row-major order, values (n_i,) f32)`` -- a sequence of such pairs (views
        into ONE pair of arrays the library returned, cut on access)."""
        batch = pssms if isinstance(pssms, MotifBatch) else MotifBatch(self, pssms, thresholds)
        if batch.protein - {seq.protein}:
            _same_alphabet(next(p for p in batch.pssms if p.protein != seq.protein), seq)
        n = len(batch)
        counts = np.zeros(n, dtype=np.uintp)
        ptr, vals = C.POINTER(Coords)(), C.POINTER(C.c_float)()
        check(self._L.lm_hip_scan_threshold_batch(self._h, batch.handles, batch.thresholds, n, seq._h,
                                                  counts.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(ptr), C.byref(vals)))
        total = int(counts.sum())
        values = self._take_array(vals, total, np.float32)
        coords = self._take_coords_array(ptr, total)
        return BatchHits(coords, values, counts)

    # -- raw device-pointer forms (used with torch tensors by bench.py / tests) -------

    def score_dptr(self, pssm: "ScoringMatrix", seq_ptr: int, seq_rows_total: int, seq_stride: int,
                   columns: int, wrap: int, length: int, row_begin: int, row_end: int,
                   out_ptr: int, out_stride: int) -> Tuple[int, int]:
        orow, mi = C.c_size_t(0), C.c_size_t(0)
        check(self._L.lm_hip_score_f32_dptr(self._h, pssm._device(self), C.c_void_p(seq_ptr),
                                            seq_rows_total, seq_stride, columns, wrap, length,
                                            row_begin, row_end, C.c_void_p(out_ptr), out_stride,
                                            C.byref(orow), C.byref(mi)))
        return orow.value, mi.value

    def argmax_dptr(self, scores_ptr: int, rows: int, stride_: int, columns: int,
                    first_cell_rule: bool = True):
        found, best, value = C.c_int(0), Coords(), C.c_float(0)
        check(self._L.lm_hip_argmax_shard_f32_dptr(self._h, C.c_void_p(scores_ptr), rows, stride_,
                                                   columns, int(first_cell_rule), C.byref(found),
                                                   C.byref(best), C.byref(value)))
        return ((best.row, best.col), float(value.value)) if found.value else None

    def _take_array(self, ptr, count: int, dtype) -> np.ndarray:
        """Wraps a malloc'ed result of the library WITHOUT copying it; the block is
        handed back to ``lm_hip_free`` when the last view of the array dies."""
        addr = C.cast(ptr, C.c_void_p).value
        if not addr or count == 0:
            if addr:
                self._L.lm_hip_free(C.c_void_p(addr))
            return np.zeros(0, dtype=dtype)
        block = _HostBlock(self._L, addr, count * np.dtype(dtype).itemsize)
        return np.asarray(block).view(dtype)

    def _take_coords_array(self, ptr, n: int) -> np.ndarray:
        # lm_hip_coords = {size_t row, col}; indices stay far below 2^63
        return self._take_array(ptr, 2 * n, np.int64).reshape(n, 2)

    def threshold_dptr(self, scores_ptr: int, rows: int, stride_: int, columns: int,
                       threshold: float) -> np.ndarray:
        """(n, 2) int64 array of (row, col) in the reference's row-major order."""
        ptr, n = C.POINTER(Coords)(), C.c_size_t(0)
        check(self._L.lm_hip_threshold_f32_dptr(self._h, C.c_void_p(scores_ptr), rows, stride_,
                                                columns, threshold, C.byref(ptr), C.byref(n)))
        return self._take_coords_array(ptr, n.value)

    # -- Score / Maximum / Threshold on u8: a DiscreteMatrix's scores ----------------------------

    def score_discrete(self, dm: "DiscreteMatrix", seq: "StripedSequence", rows: Optional[range] = None,
                       saturate: bool = True) -> Tuple[np.ndarray, int]:
        """``Score<u8, ..>::score_rows_into(&dm, &seq, rows, &mut scores)`` (pli/mod.rs:72-106):
        the u8 score matrix ``(rows, stride(C, 1))`` on the host and ``max_index``.
        ``saturate``: the SIMD back-ends' saturating adds (avx2.rs:336) or Generic's wrapping."""
        _same_alphabet(dm, seq)
        rows = range(0, seq.rows) if rows is None else rows
        n = max(rows.stop - rows.start, 0)
        st = stride(seq.columns, 1)
        out = np.zeros((n, st), dtype=np.uint8)
        orow, mi = C.c_size_t(0), C.c_size_t(0)
        check(self._L.lm_hip_score_u8(self._h, dm.data.ctypes.data, len(dm), dm.data.shape[1], dm.k,
                                      seq._h, rows.start, max(rows.stop, rows.start), int(saturate),
                                      out.ctypes.data, st, C.byref(orow), C.byref(mi)))
        return out[:orow.value], int(mi.value)

    def score_u8_dptr(self, dm: "DiscreteMatrix", seq_ptr: int, seq_rows_total: int, seq_stride: int,
                      columns: int, wrap: int, length: int, row_begin: int, row_end: int, out_ptr: int,
                      out_stride: int, saturate: bool = True) -> Tuple[int, int]:
        orow, mi = C.c_size_t(0), C.c_size_t(0)
        check(self._L.lm_hip_score_u8_dptr(self._h, dm.data.ctypes.data, len(dm), dm.data.shape[1], dm.k,
                                           C.c_void_p(seq_ptr), seq_rows_total, seq_stride, columns, wrap,
                                           length, row_begin, row_end, C.c_void_p(out_ptr), out_stride,
                                           int(saturate), C.byref(orow), C.byref(mi)))
        return int(orow.value), int(mi.value)

    def argmax_u8_dptr(self, scores_ptr: int, rows: int, stride_: int, columns: int):
        """``Maximum<u8, C>`` (pli/mod.rs:135-160): ``((row, col), value)`` or ``None``."""
        found, best, value = C.c_int(0), Coords(), C.c_uint8(0)
        check(self._L.lm_hip_argmax_u8_dptr(self._h, C.c_void_p(scores_ptr), rows, stride_, columns,
                                            C.byref(found), C.byref(best), C.byref(value)))
        return ((best.row, best.col), int(value.value)) if found.value else None

    def threshold_u8_dptr(self, scores_ptr: int, rows: int, stride_: int, columns: int, t: int) -> np.ndarray:
        """``Threshold<u8, C>`` (pli/mod.rs:210-221): (n, 2) int64 (row, col) in row-major order."""
        ptr, n = C.POINTER(Coords)(), C.c_size_t(0)
        check(self._L.lm_hip_threshold_u8_dptr(self._h, C.c_void_p(scores_ptr), rows, stride_, columns,
                                               C.c_uint8(t), C.byref(ptr), C.byref(n)))
        return self._take_coords_array(ptr, n.value)

    def score_threshold_dptr(self, pssm: "ScoringMatrix", seq_ptr: int, seq_rows_total: int,
                             seq_stride: int, columns: int, wrap: int, length: int,
                             row_begin: int, row_end: int, threshold: float):
        """Fused form: ((n, 2) int64 coords, (n,) f32 values), rows relative to row_begin."""
        ptr, vals, n = C.POINTER(Coords)(), C.POINTER(C.c_float)(), C.c_size_t(0)
        check(self._L.lm_hip_score_threshold_f32_dptr(
            self._h, pssm._device(self), C.c_void_p(seq_ptr), seq_rows_total, seq_stride, columns,
            wrap, length, row_begin, row_end, threshold, C.byref(ptr), C.byref(vals), C.byref(n)))
        return self._take_coords_array(ptr, n.value), self._take_array(vals, n.value, np.float32)

    def score_argmax_dptr(self, pssm: "ScoringMatrix", seq_ptr: int, seq_rows_total: int,
                          seq_stride: int, columns: int, wrap: int, length: int, row_begin: int,
                          row_end: int, first_cell_rule: bool = True):
        found, best, value = C.c_int(0), Coords(), C.c_float(0)
        check(self._L.lm_hip_score_argmax_shard_f32_dptr(
            self._h, pssm._device(self), C.c_void_p(seq_ptr), seq_rows_total, seq_stride, columns,
            wrap, length, row_begin, row_end, int(first_cell_rule), C.byref(found), C.byref(best),
            C.byref(value)))
        return ((best.row, best.col), float(value.value)) if found.value else None

    def stripe_dptr(self, encoded_ptr: int, length: int, columns: int, default_symbol: int,
                    wrap: int, data_ptr: int, stride_: int) -> None:
        check(self._L.lm_hip_stripe_dptr(self._h, C.c_void_p(encoded_ptr), length, columns,
                                         default_symbol, wrap, C.c_void_p(data_ptr), stride_))

    def configure_wrap_dptr(self, data_ptr: int, rows: int, stride_: int, columns: int,
                            new_wrap: int, default_symbol: int) -> None:
        check(self._L.lm_hip_configure_wrap_dptr(self._h, C.c_void_p(data_ptr), rows, stride_,
                                                 columns, new_wrap, default_symbol))

    def encode_dptr(self, ascii_ptr: int, length: int, dst_ptr: int, protein: bool = False,
                    lossy: bool = False) -> None:
        bad = C.c_size_t(0)
        st = self._L.lm_hip_encode_dptr(self._h, b"P" if protein else b"D", C.c_void_p(ascii_ptr),
                                        length, int(lossy), C.c_void_p(dst_ptr), C.byref(bad))
        if st == _ffi.ERR_INVALID_SYMBOL:
            raise InvalidSymbol(f"Invalid symbol in sequence at position {bad.value}")
        check(st)


_default: Optional[Pipeline] = None


def default_pipeline() -> Pipeline:
    """The analogue of ``Pipeline::dispatch()`` (pli/mod.rs:269-308): the reference
    re-creates a zero-sized pipeline per call (pwm/mod.rs:646, scores.rs:182); the
    GPU context it needs is cached here instead."""
    global _default
    if _default is None:
        _default = Pipeline.hip()
    return _default


# --- sequences ----------------------------------------------------------------------


def background_from_counts(counts, unknown: bool = False) -> np.ndarray:
    """``Background::from_counts`` (abc.rs:389-402) behind the filter of ``from_sequence`` / ``from_sequences``
    (abc.rs:422-456): ``counts`` is one row of ``k`` symbol counts or a ``(records, k)`` table, whose rows are summed; the
    default symbol's count is dropped unless ``unknown``; each frequency is ``count as f32 / total as f32`` with the integer
    total -- one conversion each, one f32 divide.  ``ValueError`` when nothing is left to count (``InvalidData``)."""
    table = np.asarray(counts)
    if table.dtype.kind not in "iu":
        raise TypeError("symbol counts are integers")
    table = table.astype(np.uint64 if table.dtype.kind == "u" else np.int64)
    if table.ndim == 2:
        table = table.sum(axis=0, dtype=table.dtype)
    if table.ndim != 1 or table.size < 2:
        raise ValueError("symbol counts: k entries, or a (records, k) table")
    if (table < 0).any():
        raise ValueError("symbol counts cannot be negative")
    if not unknown:
        table[-1] = 0           # abc.rs:429: `unknown || c != n`
    total = table.sum(dtype=table.dtype)
    if total == 0:
        raise ValueError("cannot build a background from a table without counts")
    return table.astype(np.float32) / total.astype(np.float32)


def markov_from_counts(symbol_counts, pair_counts, pseudocount: float = 0.0, unknown: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """A first-order chain ``(initial, transitions)`` from the symbol counts (``count_symbols``) and adjacent-pair counts
    (``count_pairs``) of a set, for ``Pipeline.sample_set``.  ``initial`` is ``background_from_counts`` of the summed symbol
    counts.  ``transitions[a][b]`` is ``pair[a][b] + pseudocount`` over the total of row ``a``: entry and total are formed in
    f64 (exact for counts), converted to f32 once each and divided in f32, as ``background_from_counts`` does.  A row without
    counts is zeros, which the sampler reads as ``initial``.  Without ``unknown`` the default symbol's row and column are
    zero."""
    initial = background_from_counts(symbol_counts, unknown)
    k = initial.size
    pairs = np.asarray(pair_counts)
    if pairs.dtype.kind not in "iu":
        raise TypeError("pair counts are integers")
    if pairs.size != k * k:
        raise ValueError(f"pair counts: a ({k}, {k}) table")
    if (pairs < 0).any():
        raise ValueError("pair counts cannot be negative")
    if not pseudocount >= 0:
        raise ValueError("a pseudocount is not negative")
    table = pairs.reshape(k, k).astype(np.float64) + float(pseudocount)
    if not unknown:
        table[-1, :] = 0
        table[:, -1] = 0
    totals = np.array([math.fsum(row) for row in table.tolist()], dtype=np.float64).astype(np.float32)
    transitions = np.zeros((k, k), dtype=np.float32)
    live = totals > 0
    transitions[live] = table[live].astype(np.float32) / totals[live, None]
    return initial, transitions


def _count_symbols(call, ctx, handle, records: int, k: int) -> np.ndarray:
    out = np.zeros(records * k, dtype=np.int64)     # (the library writes u64: a count never reaches 2^63)
    # (an empty table still needs a pointer: NULL is a misuse of the entry point, zero records are not)
    buf = out if out.size else np.zeros(1, dtype=np.int64)
    check(call(ctx, handle, buf.ctypes.data, out.size))
    return out.reshape(records, k)


def decode(symbols, protein: bool = False) -> str:
    """Symbol indices (a ``windows`` row, an ``EncodedSequence``) as text; ``ValueError`` for a byte that is no symbol, such
    as the 0xFF of an invalid window."""
    data = np.asarray(symbols, dtype=np.uint8).reshape(-1)
    table = np.frombuffer(_symbols(protein).encode("ascii"), dtype=np.uint8)
    if data.size and int(data.max()) >= table.size:
        raise ValueError(f"byte {int(data.max())} is not a symbol index")
    return table[data].tobytes().decode("ascii")


def _u64_array(values) -> np.ndarray:
    """Record numbers or positions as uint64, whatever integer type they come in (a negative one wraps, and is then invalid)."""
    a = np.asarray(values)
    if a.dtype.kind == "f" and not isinstance(values, np.ndarray) and all(isinstance(v, (int, np.integer)) for v in values):
        a = np.asarray(values, dtype=object)     # (Python ints on both sides of 2^63 become floats otherwise)
    if a.dtype == object:
        a = np.array([int(v) % (1 << 64) for v in a.reshape(-1)], dtype=np.uint64)
    elif a.dtype.kind == "i":
        a = a.astype(np.int64).view(np.uint64)
    elif a.dtype.kind == "u" or a.size == 0:
        a = a.astype(np.uint64)
    else:
        raise TypeError("records and positions are integers")
    if a.ndim != 1:
        raise ValueError("records and positions are one-dimensional")
    return a


def _site_args(sites, widths, shifts=0):
    """What ``windows`` / ``count_sites`` hand to the C ABI: ``(counts, widths, shifts, buffer, stride)``.  ``sites`` is a
    ``SetHits`` (its ``lm_hip_set_hit`` list passes as it is) or, per motif, a pair of (record, position) arrays; ``widths``
    holds one int or one matrix (its length is the width) per motif, ``shifts`` one int per motif or one for all.
    ``ValueError`` when the lengths disagree."""
    if isinstance(sites, SetHits):
        counts = np.ascontiguousarray(sites.counts, dtype=np.uintp)
        buf = np.ascontiguousarray(sites.hits)
        stride_ = buf.dtype.itemsize
    else:
        pairs = []
        for pair in sites:
            if len(pair) != 2:
                raise ValueError("a motif's sites are a pair of (record, position) arrays")
            rec, pos = _u64_array(pair[0]), _u64_array(pair[1])
            if rec.shape != pos.shape:
                raise ValueError(f"{rec.size} records against {pos.size} positions")
            pairs.append((rec, pos))
        counts = np.array([len(r) for r, _ in pairs], dtype=np.uintp)
        buf = np.zeros((int(counts.sum()), 2), dtype=np.uint64)
        if pairs:
            buf[:, 0] = np.concatenate([r for r, _ in pairs]) if buf.size else 0
            buf[:, 1] = np.concatenate([q for _, q in pairs]) if buf.size else 0
        stride_ = 16
    n = len(counts)
    if isinstance(widths, (int, np.integer)) or not hasattr(widths, "__iter__"):
        raise TypeError("widths: one int or one matrix per motif")
    w = np.array([int(x) if isinstance(x, (int, np.integer)) else len(x) for x in widths], dtype=np.uintp)
    if len(w) != n:
        raise ValueError(f"{len(w)} widths for the sites of {n} motifs")
    if (w == 0).any():
        raise ValueError("a window holds at least one symbol")
    if isinstance(shifts, (int, np.integer)):
        sh = np.full(n, int(shifts), dtype=np.int64)
    else:
        sh = np.array([int(x) for x in shifts], dtype=np.int64)
        if len(sh) != n:
            raise ValueError(f"{len(sh)} shifts for the sites of {n} motifs")
    return counts, w, sh, buf, stride_


REGION_DTYPE = np.dtype([("record", np.uint64), ("start", np.int64), ("end", np.int64), ("strand", np.uint8)], align=True)
assert REGION_DTYPE.itemsize == C.sizeof(_ffi.Region) == 32


def _strand_array(strands, n: int) -> np.ndarray:
    """0 / 1 per region from ``None`` (all plus), 0/1, booleans or ``'+'`` / ``'-'`` / ``'.'`` (a dot counts as plus)."""
    if strands is None:
        return np.zeros(n, dtype=np.uint8)
    a = np.asarray(strands)
    if a.ndim != 1:
        raise ValueError("strands are one-dimensional")
    if a.dtype.kind in "US" or a.dtype == object:
        names = {"+": 0, ".": 0, "-": 1, 0: 0, 1: 1, False: 0, True: 1}
        out = np.zeros(a.size, dtype=np.uint8)
        for i, s in enumerate(a.tolist()):
            s = s.decode("ascii", "replace") if isinstance(s, bytes) else s
            if s not in names:
                raise ValueError(f"strand {s!r}: '+', '-', '.', 0 or 1")
            out[i] = names[s]
        return out
    if a.dtype.kind not in "biu" and a.size:
        raise TypeError("strands: 0/1, booleans or '+' / '-' / '.'")
    if a.size and ((a != 0) & (a != 1)).any():
        raise ValueError("a strand is 0 or 1")
    return a.astype(np.uint8)


def _region_args(records, starts, ends, strands=None) -> np.ndarray:
    """The ``lm_hip_region`` table of ``StripedSequenceSet.regions``; ``ValueError`` when the lengths disagree."""
    rec = _u64_array(records)
    s, e = np.asarray(starts), np.asarray(ends)
    for name, a in (("starts", s), ("ends", e)):
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"{name} are integers")
        if a.ndim != 1:
            raise ValueError(f"{name} are one-dimensional")
    st = _strand_array(strands, rec.size)
    if not rec.size == s.size == e.size == st.size:
        raise ValueError(f"{rec.size} records, {s.size} starts, {e.size} ends and {st.size} strands")
    reg = np.zeros(rec.size, dtype=REGION_DTYPE)
    reg["record"], reg["start"], reg["end"], reg["strand"] = rec, s.astype(np.int64), e.astype(np.int64), st
    return reg


class RegionMap:
    """Where the records of a derived set (``StripedSequenceSet.regions``) came from: ``records`` and ``strands`` as
    they were asked for and the ``taken`` table the call returned.  Pure numpy; nothing here touches the device."""

    def __init__(self, records, taken, strands=None):
        self.records = np.asarray(records, dtype=np.int64)
        self.taken = np.asarray(taken, dtype=np.int64).reshape(-1, 2)
        self.strands = _strand_array(strands, self.records.size)
        if not self.records.size == self.taken.shape[0] == self.strands.size:
            raise ValueError("one record, one (start, end) and one strand per region")

    def __len__(self) -> int:
        return self.records.size

    def to_source(self, region_index, position, width) -> Tuple[np.ndarray, np.ndarray]:
        """A window of ``width`` symbols at ``position`` of derived record ``region_index`` (a hit of a motif of that
        length) -> ``(source record, source start)``: ``taken_start + position`` on the plus strand,
        ``taken_end - position - width`` on the minus strand, where the window reads as the reverse complement of the
        source window that starts there.  Scalars or arrays (broadcast)."""
        i = np.asarray(region_index, dtype=np.int64)
        p, w = np.asarray(position, dtype=np.int64), np.asarray(width, dtype=np.int64)
        plus = self.taken[i, 0] + p
        minus = self.taken[i, 1] - p - w
        return self.records[i], np.where(self.strands[i] == 1, minus, plus)


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else np.zeros(2, dtype=np.uint64).ctypes.data


def _symbol_index(symbol: str, protein: bool) -> int:
    i = _symbols(protein).find(symbol) if isinstance(symbol, str) and len(symbol) == 1 else -1
    if i < 0:
        raise ValueError(f"Invalid symbol: {symbol!r}")
    return i


class EncodedSequence:
    """seq.rs:83-98: a vector of symbol indices (host side; 1 byte per symbol)."""

    def __init__(self, sequence: Union[str, bytes, np.ndarray], *, protein: bool = False,
                 lossy: bool = False):
        self.protein = protein
        if isinstance(sequence, np.ndarray):
            self.data = np.ascontiguousarray(sequence, dtype=np.uint8)
            return
        raw = sequence.encode("utf-8") if isinstance(sequence, str) else bytes(sequence)
        lut = np.full(256, 255, dtype=np.uint8)
        for i, ch in enumerate(_symbols(protein)):
            lut[ord(ch)] = i
        data = lut[np.frombuffer(raw, dtype=np.uint8)]
        bad = np.flatnonzero(data == 255)
        if bad.size:
            if not lossy:  # pli/mod.rs:63 -> Err(InvalidSymbol)
                raise InvalidSymbol(f"Invalid symbol in sequence: {chr(raw[int(bad[0])])!r}")
            data[bad] = _k(protein) - 1  # seq.rs:126 unwrap_or_default
        self.data = data

    @classmethod
    def encode_lossy(cls, sequence: Union[str, bytes], *, protein: bool = False) -> "EncodedSequence":
        return cls(sequence, protein=protein, lossy=True)

    def __len__(self) -> int:
        return int(self.data.size)

    def __getitem__(self, index: int) -> int:
        """Symbol index at ``index`` (lightmotif-py lib.rs ``EncodedSequence.__getitem__``: negative
        indices count from the end, out of range raises IndexError)."""
        n = int(self.data.size)
        i = index + n if index < 0 else index
        if not 0 <= i < n:
            raise IndexError("sequence index out of range")
        return int(self.data[i])

    def __iter__(self):
        return (int(x) for x in self.data)

    def __array__(self, dtype=None, copy=None):
        """The buffer the reference exposes through ``memoryview`` (1-D, one byte per symbol)."""
        return self.data if dtype is None else self.data.astype(dtype)

    def __str__(self) -> str:
        sym = _symbols(self.protein)
        return "".join(sym[i] for i in self.data)

    def copy(self) -> "EncodedSequence":
        return EncodedSequence(self.data.copy(), protein=self.protein)

    def count_symbols(self) -> np.ndarray:
        """seq.rs:61-70 ``SymbolCount`` of the host array: ``k`` counts (int64) in alphabet order."""
        return np.bincount(self.data, minlength=_k(self.protein))[:_k(self.protein)].astype(np.int64)

    __copy__ = copy

    def stripe(self, columns: int = DEFAULT_COLUMNS) -> "StripedSequence":
        return default_pipeline().stripe(self, columns)


class StripedSequence:
    """seq.rs:288-294 ``{length, wrap, data}``, resident on the device."""

    def __init__(self, pli: Pipeline, handle: C.c_void_p, protein: bool):
        self._pli, self._h, self.protein = pli, handle, protein

    def __del__(self):
        try:
            if self._h:
                self._pli._L.lm_hip_seq_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _info(self):
        v = [C.c_size_t(0) for _ in range(5)]
        p = C.c_void_p()
        check(self._pli._L.lm_hip_seq_info(self._h, *[C.byref(x) for x in v], C.byref(p)))
        return [x.value for x in v] + [p.value or 0]

    def __len__(self) -> int:
        return self._info()[0]

    @property
    def wrap(self) -> int:
        return self._info()[1]

    @property
    def rows(self) -> int:
        """matrix().rows() - wrap()"""
        return self._info()[2]

    @property
    def stride(self) -> int:
        return self._info()[3]

    @property
    def columns(self) -> int:
        return self._info()[4]

    @property
    def data_ptr(self) -> int:
        return self._info()[5]

    def configure(self, motif: "ScoringMatrix") -> None:
        """seq.rs:362-366"""
        if len(motif) > 0:
            self.configure_wrap(len(motif) - 1)

    def configure_wrap(self, m: int) -> None:
        """seq.rs:369-381"""
        check(self._pli._L.lm_hip_seq_configure_wrap(self._pli._h, self._h, m))

    def matrix(self) -> np.ndarray:
        """Host copy of the (rows + wrap) x stride byte matrix."""
        _, wrap, rows, st, _, _ = self._info()
        out = np.empty((rows + wrap, st), dtype=np.uint8)
        check(self._pli._L.lm_hip_seq_download(self._pli._h, self._h, out.ctypes.data))
        return out

    def copy(self) -> "StripedSequence":
        """lib.rs ``StripedSequence.copy``: an independent sequence with the same rows and wrap rows."""
        length, wrap, _, _, cols, _ = self._info()
        return self._pli.upload(self.matrix(), length, wrap, cols, protein=self.protein)

    __copy__ = copy

    def count_symbols(self) -> np.ndarray:
        """seq.rs:444-483 ``SymbolCount::count_symbols`` on the device (``lm_hip_seq_count_symbols``): ``k`` counts (int64)
        in alphabet order over the positions ``p < len(self)`` -- neither the padded tail nor the wrap rows."""
        L = self._pli._L
        return _count_symbols(L.lm_hip_seq_count_symbols, self._pli._h, self._h, 1, _k(self.protein))[0]

    def count_symbol(self, symbol: str) -> int:
        """seq.rs:445-449 ``SymbolCount::count_symbol``."""
        return int(self.count_symbols()[_symbol_index(symbol, self.protein)])

    def background(self, unknown: bool = False) -> np.ndarray:
        """``Background::from_sequence`` (abc.rs:422-434) of the resident sequence: ``k`` f32 frequencies."""
        return background_from_counts(self.count_symbols(), unknown)

    def __array__(self, dtype=None, copy=None):
        """What the reference exposes through ``memoryview(striped)``: shape ``(columns, rows)`` with
        strides ``(1, stride)`` (lib.rs:303-317), i.e. indexed ``[column, row]``; a host copy here, the
        matrix lives on the device."""
        _, _, rows, _, cols, _ = self._info()
        m = self.matrix()[:rows, :cols].T
        return m if dtype is None else m.astype(dtype)


class StripedSequenceSet:
    """Many records resident as one striped sequence (``lm_hip_seqset``): ``len()`` = records."""

    header_spans: Optional[np.ndarray] = None    # (n, 2) uint64, sets made by ``Pipeline.stripe_fasta_set`` only

    def __init__(self, pli: Pipeline, handle: C.c_void_p, protein: bool):
        self._pli, self._h, self.protein = pli, handle, protein

    def __del__(self):
        try:
            if self._h:
                self._pli._L.lm_hip_seqset_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _info(self):
        v = [C.c_size_t(0) for _ in range(6)]
        check(self._pli._L.lm_hip_seqset_info(self._h, *[C.byref(x) for x in v]))
        return [x.value for x in v]

    def __len__(self) -> int:
        return self._info()[0]

    @property
    def total_length(self) -> int:
        return self._info()[1]

    @property
    def rows(self) -> int:
        return self._info()[2]

    @property
    def wrap(self) -> int:
        return self._info()[3]

    @property
    def columns(self) -> int:
        return self._info()[4]

    @property
    def lengths(self) -> np.ndarray:
        out = np.zeros(len(self), dtype=np.uintp)
        check(self._pli._L.lm_hip_seqset_lengths(self._h, out.ctypes.data, out.size))
        return out.astype(np.int64)

    def configure_wrap(self, m: int) -> None:
        """seq.rs:369-381 on the set's matrix"""
        check(self._pli._L.lm_hip_seqset_configure_wrap(self._pli._h, self._h, m))

    def count_symbols(self) -> np.ndarray:
        """``SymbolCount::count_symbols`` (seq.rs:444-483) of every record in one call (``lm_hip_seqset_count_symbols``):
        a ``(records, k)`` int64 table; row ``r`` sums to the record's length."""
        return _count_symbols(self._pli._L.lm_hip_seqset_count_symbols, self._pli._h, self._h, len(self), _k(self.protein))

    def background(self, unknown: bool = False) -> np.ndarray:
        """``Background::from_sequences`` (abc.rs:441-456) of the set's records: ``k`` f32 frequencies."""
        return background_from_counts(self.count_symbols(), unknown)

    def count_pairs(self) -> np.ndarray:
        """Adjacent-pair counts of the set (``lm_hip_seqset_count_pairs``): a ``(k, k)`` int64 table, ``[a, b]`` the number of
        positions whose symbol is ``a`` and whose successor IN THE SAME RECORD is ``b``."""
        k = _k(self.protein)
        out = np.zeros(k * k, dtype=np.int64)
        check(self._pli._L.lm_hip_seqset_count_pairs(self._pli._h, self._h, out.ctypes.data, out.size))
        return out.reshape(k, k)

    def null(self, order: int = 0, *, seed: int = 0, record_base: int = 0) -> "StripedSequenceSet":
        """A control for this set, drawn on the device (``Pipeline.sample_set``): the same record lengths and columns, and
        order 0 -- every record from its OWN composition (``count_symbols``, the default symbol included, so that N-rich
        records stay N-rich; an empty record uses no model); order 1 (DNA) -- every record from the one chain fitted on the
        whole set (``markov_from_counts`` of ``count_symbols`` and ``count_pairs``)."""
        lengths = self.lengths
        if order == 0:
            counts = self.count_symbols()
            model = counts.astype(np.float32) / np.maximum(counts.sum(axis=1), 1).astype(np.float32)[:, None]
            return self._pli.sample_set(lengths, model, seed=seed, record_base=record_base, protein=self.protein, columns=self.columns)
        if order != 1:
            raise ValueError("order 0 (i.i.d.) or 1 (first-order Markov)")
        if not lengths.any():
            initial, transitions = uniform_background(_k(self.protein)), np.zeros((_k(self.protein),) * 2, dtype=np.float32)
        else:
            counts = self.count_symbols()
            unknown = not counts[:, :-1].any()      # nothing but the default symbol: it is the model
            initial, transitions = markov_from_counts(counts, self.count_pairs(), unknown=unknown)
        return self._pli.sample_set(lengths, initial, transitions, seed=seed, record_base=record_base, protein=self.protein,
                                    columns=self.columns)

    def windows(self, sites, widths, shifts=0) -> List[Tuple[np.ndarray, np.ndarray]]:
        """The symbols of the windows ``[position + shift, position + shift + width)`` of the given sites, read out of the
        resident matrix in one call (``lm_hip_seqset_windows``): per motif a ``(count, width)`` uint8 array of symbol
        indices and a bool array ``valid``.  A window that does not lie inside its record is invalid and reads 0xFF.
        ``sites``, ``widths``, ``shifts``: see ``_site_args``."""
        counts, w, sh, buf, stride_ = _site_args(sites, widths, shifts)
        if len(counts) == 0:
            return []
        out, valid = self._windows(counts, w, sh, buf, stride_)
        res, a, b = [], 0, 0
        for c, x in zip(counts.tolist(), w.tolist()):
            res.append((out[a:a + c * x].reshape(c, x), valid[b:b + c] != 0))
            a, b = a + c * x, b + c
        return res

    def _windows(self, counts, w, sh, buf, stride_) -> Tuple[np.ndarray, np.ndarray]:
        """``lm_hip_seqset_windows`` on normalised arguments: all window bytes end to end, and one byte per site."""
        total = sum(int(c) * int(x) for c, x in zip(counts.tolist(), w.tolist()))
        out = np.empty(max(total, 1), dtype=np.uint8)
        valid = np.empty(max(int(counts.sum()), 1), dtype=np.uint8)
        keep = _ptr(buf)   # (the pointer of an empty list still has to be one)
        check(self._pli._L.lm_hip_seqset_windows(self._pli._h, self._h, counts.ctypes.data, w.ctypes.data, sh.ctypes.data, len(counts),
                                                 buf.ctypes.data if buf.size else keep, stride_, out.ctypes.data, total,
                                                 valid.ctypes.data))
        return out[:total], valid[:int(counts.sum())]

    def count_sites(self, sites, widths, shifts=0) -> Tuple[List["CountMatrix"], np.ndarray]:
        """``CountMatrix::from_sequences`` (pwm/mod.rs:209-237) over the windows of each motif's valid sites, counted on the
        device without the windows leaving it (``lm_hip_seqset_count_sites``): ``(matrices, used)`` with ``used[i]`` the
        number of valid sites of motif ``i``, which every row of matrix ``i`` sums to.  ``OverflowError`` when a count
        exceeds the u32 of a ``CountMatrix``."""
        counts, w, sh, buf, stride_ = _site_args(sites, widths, shifts)
        n, k = len(counts), _k(self.protein)
        if n == 0:
            return [], np.zeros(0, dtype=np.int64)
        entries = k * int(w.sum())
        tables = np.zeros(entries, dtype=np.uint64)
        used = np.zeros(n, dtype=np.uint64)
        keep = _ptr(buf)
        check(self._pli._L.lm_hip_seqset_count_sites(self._pli._h, self._h, counts.ctypes.data, w.ctypes.data, sh.ctypes.data, n,
                                                     buf.ctypes.data if buf.size else keep, stride_, tables.ctypes.data, entries,
                                                     used.ctypes.data))
        if tables.size and int(tables.max()) > 0xFFFFFFFF:
            raise OverflowError("a site count exceeds the u32 of a CountMatrix")
        mats, a = [], 0
        for x in w.tolist():
            mats.append(CountMatrix(tables[a:a + x * k].reshape(x, k), protein=self.protein))
            a += x * k
        return mats, used.astype(np.int64)

    def regions(self, records, starts, ends, strands=None) -> Tuple["StripedSequenceSet", np.ndarray]:
        """A set cut out of this one on the device (``lm_hip_seqset_from_regions``): record ``i`` of the result is
        ``[starts[i], ends[i])`` of record ``records[i]`` (BED: 0-based, half-open), clipped to that record, as it stands or
        -- where ``strands[i]`` is 1, ``True`` or ``'-'`` (``'+'`` and ``'.'`` count as 0; DNA only) -- as its reverse
        complement.  Returns the derived set and the ``(n, 2)`` int64 table ``taken`` of what was cut after clipping; a
        region with an unknown record, or clipped to nothing, gives an empty record and ``(0, 0)``.  ``RegionMap`` maps
        hits in the derived set back to the source."""
        reg = _region_args(records, starts, ends, strands)
        taken = np.zeros((len(reg), 2), dtype=np.uint64)
        h = C.c_void_p()
        check(self._pli._L.lm_hip_seqset_from_regions(self._pli._h, self._h, _ptr(reg), len(reg), C.byref(h), _ptr(taken)))
        return StripedSequenceSet(self._pli, h, self.protein), taken.astype(np.int64)

    def records(self) -> List["EncodedSequence"]:
        """Every record read back from the set (``StripedSequence``'s Index, seq.rs:433-442, position by position): one
        ``windows`` call with one site per non-empty record."""
        lengths = self.lengths
        live = np.flatnonzero(lengths > 0)            # (a window holds at least one symbol)
        sites = np.zeros((len(live), 2), dtype=np.uint64)
        sites[:, 0] = live
        if len(live):
            flat, valid = self._windows(np.ones(len(live), dtype=np.uintp), lengths[live].astype(np.uintp),
                                        np.zeros(len(live), dtype=np.int64), sites, 16)
            assert valid.all()
        else:
            flat = np.zeros(0, dtype=np.uint8)
        ends = np.cumsum(lengths)                     # empty records take an empty slice
        return [EncodedSequence(flat[b - n:b], protein=self.protein) for n, b in zip(lengths.tolist(), ends.tolist())]

    def record(self, r: int) -> "EncodedSequence":
        """Record ``r`` read back from the set."""
        n = len(self)
        if not -n <= r < n:
            raise IndexError("record index out of range")
        r %= n
        length = C.c_size_t(0)
        check(self._pli._L.lm_hip_seqset_record_length(self._h, r, C.byref(length)))
        if length.value == 0:
            return EncodedSequence(np.zeros(0, dtype=np.uint8), protein=self.protein)
        return EncodedSequence(self.windows([([r], [0])], [length.value])[0][0][0], protein=self.protein)


# --- matrices ------------------------------------------------------------------------


def _dict_to_rows(values: Dict[str, Iterable[float]], protein: bool, dtype) -> np.ndarray:
    sym = _symbols(protein)
    k = len(sym)
    length = None
    for key, col in values.items():
        if key not in sym:
            raise ValueError(f"Invalid symbol: {key!r}")
        col = list(col)
        if length is None:
            length = len(col)
        elif length != len(col):
            raise ValueError("Invalid number of rows")
    out = np.zeros((length or 0, k), dtype=dtype)
    for key, col in values.items():
        out[:, sym.index(key)] = np.asarray(list(col), dtype=dtype)
    return out


class CountMatrix:
    """pwm/mod.rs:178-258 (counts are M x K u32)."""

    def __init__(self, values: Union[Dict[str, Iterable[int]], np.ndarray], *, protein: bool = False):
        self.protein = protein
        self.data = (_dict_to_rows(values, protein, np.uint32) if isinstance(values, dict)
                     else np.ascontiguousarray(values, dtype=np.uint32))

    @classmethod
    def from_sequences(cls, sequences: Sequence[EncodedSequence], protein: bool = False) -> "CountMatrix":
        """pwm/mod.rs:209-237"""
        seqs = list(sequences)
        m = len(seqs[0]) if seqs else 0
        data = np.zeros((m, _k(protein)), dtype=np.uint32)
        for s in seqs:
            if len(s) != m:
                raise ValueError("Inconsistent sequence length")
            np.add.at(data, (np.arange(m), s.data), 1)
        return cls(data, protein=protein)

    def reverse_complement(self) -> "CountMatrix":
        """pwm/mod.rs:313-321: rows reversed, every symbol's column taken from its complement (A<->T, C<->G, N->N)."""
        if self.protein:
            raise ValueError("cannot complement a protein matrix")
        return CountMatrix(self.data[::-1, :5][:, [2, 3, 0, 1, 4]], protein=False)

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int) -> List[int]:
        return [int(x) for x in self.data[i]]

    def __eq__(self, other) -> bool:
        return isinstance(other, CountMatrix) and np.array_equal(self.data, other.data)

    def _to_freq(self, pseudocount: Union[None, float, Dict[str, float]]) -> np.ndarray:
        """pwm/mod.rs:240-258 ``to_freq(pseudo)`` in f32."""
        return _counts_to_freq(self.data, pseudocount, self.protein)

    def normalize(self, pseudocount: Union[None, float, Dict[str, float]] = None) -> "WeightMatrix":
        """lib.rs:501-526: ``to_freq(pseudo).to_weight(None)`` in f32."""
        f32 = np.float32
        freq = self._to_freq(pseudocount)
        bg = uniform_background(freq.shape[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(bg == 0, f32(0), freq / np.where(bg == 0, f32(1), bg)).astype(f32)  # :384-390
        return WeightMatrix(out, bg, protein=self.protein)

    def to_scoring(self, pseudocount: Union[None, float, Dict[str, float]] = None,
                   background: Union[None, Dict[str, float], np.ndarray] = None) -> "ScoringMatrix":
        """``to_freq(pseudo)`` (pwm/mod.rs:240-258) then ``into_scoring(background)`` (pwm/mod.rs:415-430): per cell
        ``log2(freq / f)`` in f32, and ``-inf`` where the background frequency ``f`` is zero.  ``background`` is a dict of
        frequencies or an array of ``k`` of them (e.g. ``background_from_counts``); ``None`` is the uniform background, and
        the result is then ``normalize(pseudocount).log_odds()`` bit for bit.  This is NOT ``log_odds(background=...)``, the
        reference's ``rescale`` (pwm/mod.rs:471-492), which makes the default symbol's column ``0 * (0 / 0) = NaN``."""
        return _freq_to_scoring(self._to_freq(pseudocount), background, self.protein)


def _counts_to_freq(counts: np.ndarray, pseudocount: Union[None, float, Dict[str, float]], protein: bool) -> np.ndarray:
    """``to_freq(pseudo)`` (pwm/mod.rs:240-258) in f32 of an ``(M, K)`` table of counts: the u32 counts of a ``CountMatrix``
    and the float64 expected counts of ``Pipeline.expected_counts_set`` take the same steps (a count is converted to f32
    first, exactly for integers below 2^24)."""
    k = counts.shape[1]
    f32 = np.float32
    if pseudocount is None:
        pseudo = np.zeros(k, dtype=f32)
    elif isinstance(pseudocount, dict):
        pseudo = _dict_to_rows({a: [b] for a, b in pseudocount.items()}, protein, f32)[0]
    else:  # abc.rs:558-573: every symbol but the default one
        pseudo = np.full(k, f32(pseudocount), dtype=f32)
        pseudo[k - 1] = 0
    out = np.zeros((len(counts), k), dtype=f32)
    for i in range(len(counts)):
        row = (counts[i].astype(f32) + pseudo).astype(f32)      # pwm/mod.rs:249-251
        total = f32(0)
        for x in row:                                            # :252 sequential f32 sum
            total = f32(total + x)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[i] = (row / total).astype(f32)                   # :253-255
    return out


def _freq_to_scoring(freq: np.ndarray, background: Union[None, Dict[str, float], np.ndarray], protein: bool) -> "ScoringMatrix":
    """``into_scoring(background)`` (pwm/mod.rs:415-430) of f32 frequencies: ``log2(freq / f)`` in f32, ``-inf`` where the
    background frequency ``f`` is zero."""
    f32 = np.float32
    k = freq.shape[1]
    if background is None:
        bg = uniform_background(k)
    elif isinstance(background, dict):
        bg = _dict_to_rows({a: [b] for a, b in background.items()}, protein, f32)[0]
    else:
        bg = np.array(background, dtype=f32)
        if bg.shape != (k,):
            raise ValueError(f"a background of {k} frequencies is needed")
    with np.errstate(divide="ignore", invalid="ignore"):
        odds = (freq / np.where(bg == 0, f32(1), bg)).astype(f32)
        out = np.where(bg == 0, f32(-np.inf), np.log2(odds, dtype=f32)).astype(f32)
    return ScoringMatrix(out, bg, protein=protein)


def expected_to_scoring(counts: np.ndarray, pseudocount: Union[None, float, Dict[str, float]] = None,
                        background: Union[None, Dict[str, float], np.ndarray] = None, *, protein: bool = False) -> "ScoringMatrix":
    """The M-step of motif EM: ``CountMatrix.to_scoring`` on an ``(M, K)`` table of float counts (the expected site counts of
    ``Pipeline.expected_counts_set``), the same f32 arithmetic: integer-valued counts give the ``CountMatrix`` result bit
    for bit."""
    counts = np.asarray(counts, dtype=np.float64)
    if counts.ndim != 2 or counts.shape[1] != _k(protein):
        raise ValueError(f"expected counts: an (M, {_k(protein)}) table")
    return _freq_to_scoring(_counts_to_freq(counts, pseudocount, protein), background, protein)


def posterior_gains(sums: "SetSums", model: str = "oops", gamma=None) -> np.ndarray:
    """The per-record gains that turn the odds of a window into its posterior (``Pipeline.expected_counts_set``), from the
    total odds ``Z`` of ``Pipeline.scan_sum_set``, ``(motifs, records)`` float64:

    ``"oops"``   one site per record: ``g = 1 / Z_r``;
    ``"zoops"``  zero or one site per record, a site with prior probability ``gamma`` (one number, or one per motif, in
                 (0, 1]): ``g = lambda_r / ((1 - gamma) + lambda_r * Z_r)``, ``lambda_r = gamma / windows_r``.

    Cells of records without a window, or whose ``Z`` is 0 or not finite, get gain 0 (the record is switched off)."""
    z = np.asarray(sums.sums, dtype=np.float64)
    windows = np.asarray(sums.windows, dtype=np.float64)
    ok = (windows > 0) & np.isfinite(z) & (z > 0)
    zs, ws = np.where(ok, z, 1.0), np.where(ok, windows, 1.0)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if model == "oops":
            g = 1.0 / zs
        elif model == "zoops":
            if gamma is None:
                raise ValueError("zoops: gamma, the prior probability of a site in a record, is needed")
            gm = np.asarray(gamma, dtype=np.float64)
            gm = gm.reshape(-1, 1) if gm.ndim else gm
            if not np.all((gm > 0) & (gm <= 1)):
                raise ValueError("zoops: gamma lies in (0, 1]")
            lam = gm / ws
            g = lam / ((1.0 - gm) + lam * zs)
        else:
            raise ValueError(f"model {model!r}: 'oops' or 'zoops'")
    return np.ascontiguousarray(np.where(ok & np.isfinite(g), g, 0.0), dtype=np.float64)


def _em_likelihood(sums: "SetSums", gains: np.ndarray, model: str, gamma):
    """``(log2-likelihood ratio per motif, new gamma per motif or None)`` of ``Pipeline.em_step`` from the total odds and the
    gains made of them: over the records that are switched on, ``log2 Z_r`` (OOPS) or ``log2((1 - gamma) + lambda_r Z_r)``
    (ZOOPS), and for ZOOPS the mean posterior mass ``g_r Z_r`` per record with a window."""
    live = gains > 0
    z = np.where(live, sums.sums, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if model == "oops":
            return np.log2(z).sum(axis=1), None
        gm = np.asarray(gamma, dtype=np.float64)
        gm = gm.reshape(-1, 1) if gm.ndim else gm
        lam = gm / np.maximum(sums.windows, 1)
        ll = np.where(live, np.log2((1.0 - gm) + lam * z), 0.0).sum(axis=1)
        has = np.maximum((sums.windows > 0).sum(axis=1), 1)
        return ll, np.minimum(np.where(live, gains * z, 0.0).sum(axis=1) / has, 1.0)


def uniform_background(k: int) -> np.ndarray:
    """abc.rs:473-487: 1/(K-1) everywhere, 0 for the default symbol."""
    bg = np.full(k, np.float32(1) / np.float32(k - 1), dtype=np.float32)
    bg[k - 1] = 0
    return bg


class WeightMatrix:
    """pwm/mod.rs:450-456: odds ratios."""

    def __init__(self, data: np.ndarray, background: np.ndarray, *, protein: bool = False):
        self.data = np.ascontiguousarray(data, dtype=np.float32)
        self.background = np.asarray(background, dtype=np.float32)
        self.protein = protein

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int) -> List[float]:
        return [float(x) for x in self.data[i]]

    def __eq__(self, other) -> bool:
        return (isinstance(other, WeightMatrix) and self.protein == other.protein
                and np.array_equal(self.data, other.data, equal_nan=True))

    def log_odds(self, background: Optional[Dict[str, float]] = None, base: float = 2.0) -> "ScoringMatrix":
        """lib.rs WeightMatrix.log_odds -> rescale + to_scoring_with_base (pwm/mod.rs:505-526)."""
        data, bg = self.data, self.background
        if background is not None:
            nb = _dict_to_rows({a: [b] for a, b in background.items()}, self.protein, np.float32)[0]
            with np.errstate(divide="ignore", invalid="ignore"):
                data = (data * (bg / nb)).astype(np.float32)  # pwm/mod.rs:477-481
            bg = nb
        with np.errstate(divide="ignore"):
            if base == 2.0:
                out = np.log2(data, dtype=np.float32)
            elif base == 10.0:
                out = np.log10(data, dtype=np.float32)
            else:
                out = (np.log(data, dtype=np.float32) / np.log(np.float32(base))).astype(np.float32)
        return ScoringMatrix(out, bg, protein=self.protein)


class ScoringMatrix:
    """pwm/mod.rs:561-564 ``{background, data: DenseMatrix<f32, K>}``.

    ``data`` is kept in the reference's padded layout (M x stride(K) f32: stride 8
    for DNA, 24 for protein) so the pointer handed to the C ABI is what a Rust
    caller would hand over."""

    def __init__(self, values: Union[Dict[str, Iterable[float]], np.ndarray],
                 background: Union[None, Dict[str, float], np.ndarray] = None, *,
                 protein: bool = False):
        self.protein = protein
        k = _k(protein)
        dense = (_dict_to_rows(values, protein, np.float32) if isinstance(values, dict)
                 else np.asarray(values, dtype=np.float32))
        if dense.ndim != 2 or dense.shape[1] < k:
            raise ValueError("scoring matrix must be M x K")
        st = stride(k, 4)
        self.data = np.zeros((dense.shape[0], st), dtype=np.float32)  # dense.rs:144-147
        self.data[:, :k] = dense[:, :k]
        if isinstance(background, dict):
            background = _dict_to_rows({a: [b] for a, b in background.items()}, protein, np.float32)[0]
        self.background = uniform_background(k) if background is None else np.asarray(background, np.float32)
        self._dev: Dict[int, C.c_void_p] = {}
        self._plis: Dict[int, Pipeline] = {}

    @property
    def k(self) -> int:
        return _k(self.protein)

    def __len__(self) -> int:
        return self.data.shape[0]

    def __getitem__(self, i: int) -> List[float]:
        """Row ``i``: the K scores of motif position ``i`` (lib.rs ``ScoringMatrix.__getitem__``)."""
        n = self.data.shape[0]
        j = i + n if i < 0 else i
        if not 0 <= j < n:
            raise IndexError("list index out of range")
        return [float(x) for x in self.data[j, :self.k]]

    def __eq__(self, other) -> bool:
        return (isinstance(other, ScoringMatrix) and self.protein == other.protein
                and np.array_equal(self.data, other.data, equal_nan=True))

    def _device(self, pli: Pipeline) -> C.c_void_p:
        key = id(pli)
        if key not in self._dev:
            h = C.c_void_p()
            check(pli._L.lm_hip_pssm_create(pli._h, self.data.ctypes.data, self.data.shape[0],
                                            self.data.shape[1], self.k, C.byref(h)))
            self._dev[key] = h
            self._plis[key] = pli
        return self._dev[key]

    def __del__(self):
        try:
            for key, h in self._dev.items():
                self._plis[key]._L.lm_hip_pssm_destroy(h)
        except Exception:
            pass

    def calculate(self, sequence: StripedSequence) -> "StripedScores":
        """lib.rs:855-874: ``configure(pssm)`` then full-range ``pli.score``."""
        if sequence.protein != self.protein:
            raise ValueError("alphabet mismatch")
        sequence.configure(self)
        return sequence._pli.score(self, sequence)

    def score(self, sequence: StripedSequence) -> "StripedScores":
        """pwm/mod.rs:640-648 (the caller configures the wrap rows, like in Rust)."""
        return sequence._pli.score(self, sequence)

    def _extreme_score(self, pick) -> float:
        total = np.float32(0.0)
        for row in self.data[:, :self.k - 1]:      # the default symbol (N / X) is left out
            total = np.float32(total + pick(row))
        return float(total)

    def min_score(self) -> float:
        """pwm/mod.rs:592-602: sum over positions of the lowest weight (f32, in row order)."""
        return self._extreme_score(np.min)

    def max_score(self) -> float:
        """pwm/mod.rs:605-615: sum over positions of the highest weight."""
        return self._extreme_score(np.max)

    def to_discrete(self) -> "DiscreteMatrix":
        """pwm/mod.rs:665-696: u8 weights that over-estimate the scores, in f32 arithmetic like
        the reference (row offsets = row minima over the K-1 real symbols with -inf counted
        as -max_score, one global factor = (max_score - offset) / 255, weights rounded UP and
        converted with Rust's saturating ``as u8``)."""
        k = self.k
        p = self.data[:, :k]
        max_score = np.float32(self.max_score())
        offsets = np.empty(len(self), np.float32)
        for j in range(len(self)):
            row = np.where(np.isinf(p[j, :k - 1]), np.float32(-max_score), p[j, :k - 1])
            offsets[j] = row.min()
        offset = np.float32(0.0)
        for x in offsets:
            offset = np.float32(offset + x)
        factor = np.float32(np.float32(max_score - offset) / np.float32(255))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            scaled = np.ceil((p - offsets[:, None]).astype(np.float32) / factor)
            scaled = np.where(np.isnan(scaled), np.float32(0), np.clip(scaled, 0, 255))
        data = np.zeros((len(self), stride(k, 1)), dtype=np.uint8)  # DenseMatrix<u8, K>
        data[:, :k] = scaled.astype(np.uint8)
        return DiscreteMatrix(data, float(factor), offsets, float(offset), protein=self.protein)

    @property
    def score_distribution(self):
        """pwm/mod.rs:698-705 ``to_score_distribution`` (MEME-style, pwm/dist.rs)."""
        from .dist import ScoreDistribution
        if getattr(self, "_dist", None) is None:
            self._dist = ScoreDistribution(self)
        return self._dist

    def pvalue(self, score: float, method: str = "meme") -> float:
        """lib.pyi ``ScoringMatrix.pvalue``; only the MEME method is on this path
        (TFM-PVALUE is a separate GPL crate, out of scope)."""
        if method != "meme":
            raise ValueError(f"unsupported method: {method!r}")
        return self.score_distribution.pvalue(score)

    def score_for_pvalue(self, pvalue: float, method: str = "meme") -> float:
        """lib.pyi ``ScoringMatrix.score`` (renamed here: ``score`` is the scoring call)."""
        if method != "meme":
            raise ValueError(f"unsupported method: {method!r}")
        return self.score_distribution.score(pvalue)

    def reverse_complement(self) -> "ScoringMatrix":
        """pwm/mod.rs:566-577 (DNA: A<->T, C<->G, N->N).  Device copies of ``self`` get their
        complement made by the library (``lm_hip_pssm_reverse_complement``), without an upload."""
        if self.protein:
            raise ValueError("cannot complement a protein matrix")
        comp = [2, 3, 0, 1, 4]
        rc = ScoringMatrix(self.data[::-1, :5][:, comp], self.background, protein=False)
        for key, h in self._dev.items():
            pli = self._plis[key]
            out = C.c_void_p()
            check(pli._L.lm_hip_pssm_reverse_complement(pli._h, h, C.byref(out)))
            rc._dev[key], rc._plis[key] = out, pli
        return rc


class DiscreteMatrix:
    """pwm/mod.rs:754-791 ``{data: DenseMatrix<u8, K>, factor, offsets, offset}``."""

    def __init__(self, data: np.ndarray, factor: float, offsets: np.ndarray, offset: float, *,
                 protein: bool = False):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.factor, self.offsets, self.offset, self.protein = factor, offsets, offset, protein

    @property
    def k(self) -> int:
        return _k(self.protein)

    def __len__(self) -> int:
        return self.data.shape[0]

    def scale(self, score: float) -> int:
        """pwm/mod.rs:777-779: rounds DOWN (f32 -> u8 threshold), saturating ``as u8``."""
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v = np.floor(np.float32(np.float32(score) - np.float32(self.offset)) / np.float32(self.factor))
        return 0 if v != v else int(min(max(v, 0), 255))

    def unscale(self, score: int) -> float:
        """pwm/mod.rs:783-785"""
        return float(np.float32(np.float32(score) * np.float32(self.factor) + np.float32(self.offset)))


class MotifBatch:
    """Device handles (+ thresholds) of a motif list, as arrays the C ABI reads (Pipeline.prepare_batch)."""

    def __init__(self, pli: "Pipeline", pssms: Sequence["ScoringMatrix"], thresholds: Optional[Sequence[float]] = None):
        self.pssms = list(pssms)          # (keeps the matrices, hence their device tables, alive)
        self.protein = {p.protein for p in self.pssms}  # the alphabets present (checked against each sequence)
        n = len(self.pssms)
        self.handles = (C.c_void_p * n)(*[p._device(pli) for p in self.pssms])
        self.thresholds = None
        if thresholds is not None:
            ts = np.ascontiguousarray(thresholds, dtype=np.float32)
            if ts.shape != (n,):
                raise ValueError("one threshold per motif")
            self._ts = ts
            self.thresholds = ts.ctypes.data_as(C.POINTER(C.c_float))

    def __len__(self) -> int:
        return len(self.pssms)


class BatchHits(Sequence):
    """The result of a batched fused threshold scan: per motif ``(coords (n_i, 2) int64, values (n_i,) f32)``, cut out of
    the two arrays the library returned when an element is asked for (2 346 slices cost a millisecond the scan does not)."""

    def __init__(self, coords: np.ndarray, values: np.ndarray, counts: np.ndarray):
        self.coords, self.values, self.counts = coords, values, counts
        self._starts = np.concatenate(([0], np.cumsum(counts, dtype=np.int64)))

    def __len__(self) -> int:
        return len(self.counts)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        a, b = int(self._starts[i]), int(self._starts[i + 1])
        return self.coords[a:b], self.values[a:b]

    @property
    def total(self) -> int:
        return int(self._starts[-1])


SET_HIT_DTYPE = np.dtype({"names": ["record", "position", "score"], "formats": [np.int64, np.int64, np.float32],
                          "offsets": [0, 8, 16], "itemsize": C.sizeof(SetHit)})   # lm_hip_set_hit


class SetHits(Sequence):
    """The result of a scan over a sequence set: per motif ``(records int64, positions int64, scores f32)``, cut out of the
    ONE array of ``lm_hip_set_hit`` the library returned when an element is asked for (as ``BatchHits``)."""

    def __init__(self, hits: np.ndarray, counts: np.ndarray):
        self.hits, self.counts = hits, counts
        self._starts = np.concatenate(([0], np.cumsum(counts, dtype=np.int64)))

    def __len__(self) -> int:
        return len(self.counts)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        h = self.hits[int(self._starts[i]):int(self._starts[i + 1])]
        return h["record"], h["position"], h["score"]

    @property
    def total(self) -> int:
        return int(self._starts[-1])


SET_BEST_DTYPE = np.dtype({"names": ["position", "score", "found"], "formats": [np.uint64, np.float32, np.int32],
                           "offsets": [0, 8, 12], "itemsize": C.sizeof(_ffi.SetBest)})   # lm_hip_set_best


class SetBest:
    """The result of ``Pipeline.scan_best_set``: three ``(motifs, records)`` arrays -- ``found`` (bool), ``position``
    (int64, -1 where not found) and ``score`` (float32, NaN where not found); ``last_kernel`` names the kernel that ran
    last for the call ("" when nothing ran)."""

    def __init__(self, raw: np.ndarray, last_kernel: str = ""):
        self.raw = raw                                   # (motifs, records) of lm_hip_set_best
        self.found = raw["found"] != 0
        self.position = np.where(self.found, raw["position"].astype(np.int64), np.int64(-1))
        self.score = np.where(self.found, raw["score"], np.float32(np.nan)).astype(np.float32)
        self.last_kernel = last_kernel

    @property
    def shape(self) -> Tuple[int, int]:
        return self.raw.shape

    def __len__(self) -> int:
        return self.raw.shape[0]


class SetCounts:
    """The result of ``Pipeline.scan_count_set``: ``counts`` -- ``(motifs, levels, records)`` uint32, the windows of a motif
    in a record that reach a cut-off -- and ``windows`` -- ``(motifs, records)`` int64, the windows there are,
    ``max(0, L_r - M_i + 1)``, made on the host from the record lengths; ``last_kernel`` names the kernel that ran last for
    the call ("" when nothing ran)."""

    def __init__(self, counts: np.ndarray, windows: np.ndarray, last_kernel: str = ""):
        self.counts, self.windows, self.last_kernel = counts, windows, last_kernel

    @property
    def shape(self) -> Tuple[int, int, int]:
        return self.counts.shape

    def __len__(self) -> int:
        return self.counts.shape[0]


class SetSums:
    """The result of ``Pipeline.scan_sum_set``: ``sums`` -- ``(motifs, records)`` float64, the total odds of a motif in a
    record -- and ``windows`` -- ``(motifs, records)`` int64, the windows there are, ``max(0, L_r - M_i + 1)``, made on
    the host from the record lengths; ``last_kernel`` names the kernel that ran last for the call ("" when nothing ran)."""

    def __init__(self, sums: np.ndarray, windows: np.ndarray, last_kernel: str = ""):
        self.sums, self.windows, self.last_kernel = sums, windows, last_kernel

    @property
    def shape(self) -> Tuple[int, int]:
        return self.sums.shape

    def __len__(self) -> int:
        return self.sums.shape[0]

    def mean(self) -> np.ndarray:
        """The average odds per window, NaN where a record has no window."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.windows > 0, self.sums / np.maximum(self.windows, 1), np.nan)

    def log2(self) -> np.ndarray:
        """log2 of the total odds: -inf where the sum is 0."""
        with np.errstate(divide="ignore"):
            return np.log2(self.sums)


class SetExpectedCounts:
    """The result of ``Pipeline.expected_counts_set``: ``counts`` -- per motif an ``(M_i, K)`` float64 table of expected
    symbol counts, exact multiples of ``2 ** -frac_bits`` --, ``frac_bits`` -- the fixed point of the set -- and ``kernel``
    -- the kernel that ran last for the call ("" when nothing ran)."""

    def __init__(self, counts: List[np.ndarray], frac_bits: int, kernel: str = ""):
        self.counts, self.frac_bits, self.kernel = counts, frac_bits, kernel

    def __len__(self) -> int:
        return len(self.counts)

    def quanta(self) -> List[np.ndarray]:
        """The tables as the integers the device summed: ``counts * 2 ** frac_bits``, int64."""
        return [np.ldexp(c, self.frac_bits).astype(np.int64) for c in self.counts]


VARIANT_DTYPE = np.dtype({"names": ["record", "position", "alt"], "formats": [np.uint64, np.uint64, np.uint8],
                          "offsets": [0, 8, 16], "itemsize": C.sizeof(_ffi.Variant)})   # lm_hip_variant
VARIANT_EFFECT_DTYPE = np.dtype([("ref_score", np.float32), ("alt_score", np.float32), ("ref_back", np.uint32),
                                 ("alt_back", np.uint32)])                               # lm_hip_variant_effect
VARIANT_HIT_DTYPE = np.dtype([("variant", np.uint64), ("effect", VARIANT_EFFECT_DTYPE)])  # lm_hip_variant_hit


def _variant_starts(position: np.ndarray, back: np.ndarray) -> np.ndarray:
    """Record-relative window starts ``position - back``, -1 where ``back`` says none."""
    none = back == _ffi.VARIANT_NONE
    return np.where(none, np.int64(-1), (position - np.where(none, 0, back).astype(np.uint64)).astype(np.int64))


class SetVariantEffects:
    """The result of ``Pipeline.scan_variants_set``: ``ref_score`` / ``alt_score`` -- ``(motifs, variants)`` float32, NaN
    where the allele has no (non-NaN) window -- ``ref_position`` / ``alt_position`` -- int64 record-relative window STARTS,
    -1 for none, made from ``raw`` when asked for -- ``ref_symbol`` -- ``(variants,)`` uint8, the resident symbol, 255 for an invalid variant -- and ``valid``;
    ``last_kernel`` names the kernel that ran last for the call ("" when nothing ran)."""

    def __init__(self, raw: np.ndarray, variants: np.ndarray, ref_symbol: np.ndarray, last_kernel: str = ""):
        self.raw = raw                                   # (motifs, variants) of lm_hip_variant_effect
        self.ref_score, self.alt_score = raw["ref_score"], raw["alt_score"]
        self._variants = variants
        self.ref_symbol = ref_symbol
        self.valid = ref_symbol != 255
        self.last_kernel = last_kernel

    @property
    def ref_position(self) -> np.ndarray:
        return _variant_starts(self._variants["position"].reshape(1, -1), self.raw["ref_back"])

    @property
    def alt_position(self) -> np.ndarray:
        return _variant_starts(self._variants["position"].reshape(1, -1), self.raw["alt_back"])

    @property
    def shape(self) -> Tuple[int, int]:
        return self.raw.shape

    def __len__(self) -> int:
        return self.raw.shape[0]


class SetVariantHits(Sequence):
    """The result of ``Pipeline.scan_variant_hits_set``: per motif a structured array (``variant`` -- the index into the
    caller's list -- ``ref_score``, ``alt_score``, ``ref_position``, ``alt_position`` as in ``SetVariantEffects``), cut out
    of the ONE array of ``lm_hip_variant_hit`` the library returned when an element is asked for (as ``SetHits``);
    ``counts``, ``total``, ``ref_symbol`` and ``valid`` per variant of the call."""

    DTYPE = np.dtype([("variant", np.int64), ("ref_score", np.float32), ("alt_score", np.float32), ("ref_position", np.int64),
                      ("alt_position", np.int64)])

    def __init__(self, hits: np.ndarray, counts: np.ndarray, variants: np.ndarray, ref_symbol: np.ndarray, last_kernel: str = ""):
        self.hits, self.counts, self.variants = hits, counts, variants
        self.ref_symbol, self.valid, self.last_kernel = ref_symbol, ref_symbol != 255, last_kernel
        self._starts = np.concatenate(([0], np.cumsum(counts, dtype=np.int64)))

    def __len__(self) -> int:
        return len(self.counts)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        h = self.hits[int(self._starts[i]):int(self._starts[i + 1])]
        out = np.zeros(len(h), dtype=self.DTYPE)
        position = self.variants["position"][h["variant"].astype(np.int64)]
        out["variant"], out["ref_score"], out["alt_score"] = h["variant"], h["effect"]["ref_score"], h["effect"]["alt_score"]
        out["ref_position"] = _variant_starts(position, h["effect"]["ref_back"])
        out["alt_position"] = _variant_starts(position, h["effect"]["alt_back"])
        return out

    @property
    def total(self) -> int:
        return int(self._starts[-1])


class ScoreDistributions:
    """The resident score distributions of ``n`` motifs (``Pipeline.score_distributions``; ``lm_hip_dists``).
    ``scale``, ``offset`` (float64, whole numbers), ``min_score``, ``max_score`` (int64) and ``rows`` are arrays with one
    entry per motif, the parameters ``dist.ScoreDistribution`` keeps (dist.rs:133-161, 197-213)."""

    def __init__(self, pli: Pipeline, pssms: Sequence["ScoringMatrix"]):
        self._pli, self._L = pli, pli._L
        self.pssms = list(pssms)              # (keeps the matrices, hence their device tables, alive)
        n = len(self.pssms)
        for p in self.pssms:
            if p.background.shape != (p.k,):
                raise ValueError("a background has one frequency per symbol")
        handles = (C.c_void_p * n)(*[p._device(pli) for p in self.pssms])
        bgs = [np.ascontiguousarray(p.background, dtype=np.float32) for p in self.pssms]
        bg_ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bgs])
        self._h = C.c_void_p()
        check(self._L.lm_hip_dists_create(pli._h, handles, n, bg_ptrs, C.byref(self._h)))
        self.rows = np.zeros(n, dtype=np.int64)
        self.scale, self.offset = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        self.min_score, self.max_score = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        rows, sc, off, lo, hi = C.c_size_t(0), C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int64(0)
        for i in range(n):
            check(self._L.lm_hip_dists_info(self._h, i, C.byref(rows), C.byref(sc), C.byref(off), C.byref(lo), C.byref(hi), None))
            self.rows[i], self.scale[i], self.offset[i] = rows.value, sc.value, off.value
            self.min_score[i], self.max_score[i] = lo.value, hi.value

    def __del__(self):
        try:
            if self._h:
                self._L.lm_hip_dists_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def __len__(self) -> int:
        return len(self.pssms)

    def sf(self, i: int) -> np.ndarray:
        """The survival function of motif ``i``: float64, ``1000 * M + 1`` entries (``lm_hip_dists_sf``)."""
        n = len(self)
        j = i + n if i < 0 else i
        if not 0 <= j < n:
            raise IndexError(i)
        out = np.empty(int(self.rows[j]) * 1000 + 1, dtype=np.float64)
        check(self._L.lm_hip_dists_sf(self._pli._h, self._h, j, out.ctypes.data, out.size))
        return out

    def distribution(self, i: int):
        """Motif ``i``'s distribution as a ``dist.ScoreDistribution`` around the downloaded table."""
        from .dist import ScoreDistribution
        n = len(self)
        j = i + n if i < 0 else i
        return ScoreDistribution.from_parts(self.sf(j), self.scale[j], int(self.offset[j]), int(self.rows[j]),
                                            int(self.min_score[j]), int(self.max_score[j]))

    def thresholds(self, pvalue) -> np.ndarray:
        """``ScoreDistribution.score`` (dist.rs:104-116) of every motif in one call: float32 ``[n]`` for one p-value, or
        for one p-value per motif."""
        n = len(self)
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(pvalue, dtype=np.float64), (n,)))
        out = np.zeros(n, dtype=np.float32)
        check(self._L.lm_hip_dists_scores(self._pli._h, self._h, p.ctypes.data if n else None, out.ctypes.data if n else None))
        return out

    def pvalues(self, counts, scores=None) -> np.ndarray:
        """``ScoreDistribution.pvalue`` (dist.rs:91-101) of many scores in one call: float64, one per score.  Either
        ``(counts, scores)`` -- ``counts[i]`` consecutive float32 scores belong to motif ``i`` -- or the ``SetHits`` /
        ``BatchHits`` of a scan of the same motifs, whose score column is read where it lies."""
        if scores is None:
            hits = counts
            counts = hits.counts
            scores = hits.hits["score"] if isinstance(hits, SetHits) else hits.values
        counts = np.ascontiguousarray(counts, dtype=np.uintp)
        if counts.shape != (len(self),):
            raise ValueError("one count per motif")
        scores = np.asarray(scores)
        if scores.dtype != np.float32 or scores.ndim != 1 or (scores.size > 1 and scores.strides[0] < 4):
            scores = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
        total = int(counts.sum())
        if scores.size != total:
            raise ValueError(f"{total} scores counted, {scores.size} given")
        out = np.zeros(total, dtype=np.float64)
        if total:
            check(self._L.lm_hip_dists_pvalues(self._pli._h, self._h, counts.ctypes.data, scores.ctypes.data,
                                               scores.strides[0] if total > 1 else 4, out.ctypes.data))
        return out


# --- scores -----------------------------------------------------------------------------


class StripedScores:
    """scores.rs:102-107 ``{data, max_index}``, resident on the device."""

    def __init__(self, pli: Pipeline, handle: C.c_void_p):
        self._pli, self._h = pli, handle

    @classmethod
    def empty(cls, pli: Optional[Pipeline] = None, columns: int = DEFAULT_COLUMNS) -> "StripedScores":
        pli = pli or default_pipeline()
        h = C.c_void_p()
        check(pli._L.lm_hip_scores_create(pli._h, columns, C.byref(h)))
        return cls(pli, h)

    def __del__(self):
        try:
            if self._h:
                self._pli._L.lm_hip_scores_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _info(self):
        v = [C.c_size_t(0) for _ in range(4)]
        p = C.c_void_p()
        check(self._pli._L.lm_hip_scores_info(self._h, *[C.byref(x) for x in v], C.byref(p)))
        return [x.value for x in v] + [p.value or 0]

    @property
    def rows(self) -> int:
        return self._info()[0]

    @property
    def stride(self) -> int:
        return self._info()[1]

    @property
    def columns(self) -> int:
        return self._info()[2]

    @property
    def max_index(self) -> int:
        return self._info()[3]

    @property
    def data_ptr(self) -> int:
        return self._info()[4]

    def set_first_cell_rule(self, enabled: bool) -> None:
        """This StripedScores is a row shard of a larger matrix: ``enabled=False`` when it does
        not hold the matrix's first row (Maximum::argmax's NaN first-cell rule is skipped)."""
        check(self._pli._L.lm_hip_scores_set_first_cell_rule(self._h, int(bool(enabled))))

    def is_empty(self) -> bool:
        return self.rows == 0

    def matrix(self) -> np.ndarray:
        """Host copy of the rows x stride f32 matrix."""
        rows, st = self.rows, self.stride
        out = np.empty((rows, st), dtype=np.float32)
        check(self._pli._L.lm_hip_scores_download(self._pli._h, self._h, out.ctypes.data))
        return out

    def __array__(self, dtype=None, copy=None) -> np.ndarray:
        """``numpy.asarray(scores)``: the reference exports the matrix through the buffer
        protocol as a read-only (columns, rows) view with strides (4, stride * 4)
        (lib.rs:1051-1085, 1129-1139), i.e. ``a[col, row]`` -- flattened in C order that is
        the score of every position ``col * rows + row`` in sequence order."""
        a = self.matrix()[:, :self.columns].T
        a.flags.writeable = False
        return a if dtype is None else a.astype(dtype)

    def offset(self, row: int, col: int) -> int:
        """scores.rs:155-157"""
        return col * self.rows + row

    def __len__(self) -> int:
        """scores.rs:274-279: min(max_index, rows * C)"""
        rows, _, cols, mi, _ = self._info()
        return min(mi, rows * cols)

    def unstripe(self) -> np.ndarray:
        """scores.rs:167-170"""
        m = self.matrix()
        n, rows = len(self), self.rows
        i = np.arange(n)
        return m[i % rows, i // rows] if rows else np.zeros(0, np.float32)

    def __iter__(self) -> Iterator[float]:
        return iter(float(x) for x in self.unstripe())

    def __getitem__(self, index: int) -> float:
        """scores.rs:246-254 (lib.rs:1038-1050 raises IndexError past the end)."""
        n = len(self)
        if index < 0:
            index += n
        if not 0 <= index < n:
            raise IndexError(index)
        rows = self.rows
        return float(self.rows_matrix(index % rows, index % rows + 1)[0, index // rows])

    def rows_matrix(self, row_begin: int, row_end: int) -> np.ndarray:
        """Host copy of rows ``[row_begin, row_end)`` only (``(n, stride)`` f32)."""
        out = np.empty((max(row_end - row_begin, 0), self.stride), dtype=np.float32)
        check(self._pli._L.lm_hip_scores_download_rows(self._pli._h, self._h, row_begin, row_end,
                                                       out.ctypes.data))
        return out

    def argmax(self) -> Optional[int]:
        """scores.rs:190-192"""
        mc = self._pli.argmax(self)
        return None if mc is None else self.offset(*mc)

    def max(self) -> Optional[float]:
        """scores.rs:181-183"""
        return self._pli.max(self)

    def threshold(self, threshold: float) -> List[int]:
        """scores.rs:207-213 (unsorted: row-major order of the striped matrix)."""
        rows = self.rows
        return [c * rows + r for r, c in self._pli.threshold(self, threshold)]


# --- Scanner (scan.rs:96-250 semantics on the fused kernel) ----------------------------------


class Hit:
    """scan.rs:52-75"""

    __slots__ = ("position", "score")

    def __init__(self, position: int, score: float):
        self.position, self.score = position, score

    def __repr__(self) -> str:
        return f"Hit(position={self.position}, score={self.score})"


# lm_hip_hit {size_t position; float score;} as the C compiler lays it out
_HIT_DTYPE = np.dtype({"names": ["position", "score"], "formats": ["<u8", "<f4"],
                       "offsets": [_ffi.Hit.position.offset, _ffi.Hit.score.offset],
                       "itemsize": C.sizeof(_ffi.Hit)})


class Scanner:
    """All positions with ``score >= threshold`` and ``position + M <= L``
    (scan.rs:185-190), found by the fused score+threshold kernel: a packed u16
    discrete prefilter (the device form of scan.rs:169-178's DiscreteMatrix) with exact
    f32 re-scoring of the candidates.

    Iteration yields the hits in the reference's order: blocks of ``block_size`` rows in
    ascending order (scan.rs:174-176, 196), and inside a block the LAST cell in row-major
    (row, col) order first -- the reference pushes a block's hits in ``Threshold`` order and
    pops them from the end of the vector (scan.rs:184-198).  ``positions`` / ``scores`` hold
    the same hits in ascending position, as the device returns them."""

    def __init__(self, pssm: ScoringMatrix, sequence: StripedSequence, threshold: float = 0.0,
                 block_size: int = 256):
        if pssm.protein != sequence.protein:
            raise ValueError("motif and sequence alphabets differ")
        if block_size < 1:
            raise ValueError("block_size must be positive")
        self.block_size = block_size
        self.threshold = threshold
        if sequence.wrap < len(pssm) - 1:  # scan.rs:127-131 panics
            raise ValueError(f"not enough wrapping rows for motif of length {len(pssm)}")
        self._pssm, self._seq = pssm, sequence
        self._positions: Optional[np.ndarray] = None  # filled by the first use (one fused scan)
        self._scores: Optional[np.ndarray] = None
        self._order: Optional[np.ndarray] = None
        self._next = 0

    def _scan(self, threshold: float) -> Tuple[np.ndarray, np.ndarray]:
        pli = self._seq._pli
        ptr, n = C.POINTER(_ffi.Hit)(), C.c_size_t(0)
        check(pli._L.lm_hip_scan_f32(pli._h, self._pssm._device(pli), self._seq._h, threshold,
                                     C.byref(ptr), C.byref(n)))
        try:
            raw = np.frombuffer(C.string_at(ptr, n.value * C.sizeof(_ffi.Hit)) if n.value else b"",
                                dtype=_HIT_DTYPE)
        finally:
            if ptr:
                pli._L.lm_hip_free(ptr)
        return raw["position"].astype(np.int64), raw["score"].astype(np.float32)

    def _collect(self) -> None:
        if self._order is not None:
            return
        self._positions, self._scores = self._scan(self.threshold)
        rows = max(self._seq.rows, 1)
        row, col = self._positions % rows, self._positions // rows
        # yield order: block ascending, then (row, col) descending
        self._order = np.lexsort((-col, -row, row // self.block_size))

    @property
    def positions(self) -> np.ndarray:
        """The hits' positions in ascending order (int64)."""
        self._collect()
        return self._positions

    @property
    def scores(self) -> np.ndarray:
        """The f32 scores of ``positions``."""
        self._collect()
        return self._scores

    def __iter__(self) -> "Scanner":
        return self

    def __next__(self) -> Hit:
        self._collect()
        if self._next >= self._order.size:
            raise StopIteration
        i = self._order[self._next]
        self._next += 1
        return Hit(int(self._positions[i]), float(self._scores[i]))

    def __len__(self) -> int:
        """Hits not yet yielded."""
        self._collect()
        return int(self._order.size - self._next)

    @staticmethod
    def _best(pos: np.ndarray, sc: np.ndarray) -> Optional[Hit]:
        if sc.size == 0:
            return None
        top = np.nonzero(sc == sc.max())[0]
        i = top[np.argmax(pos[top])]
        return Hit(int(pos[i]), float(sc[i]))

    def max(self, saturate: bool = True, strict_reference: Optional[bool] = None) -> Optional[Hit]:
        """``Scanner::max`` exactly as the reference computes it (scan.rs:200-249); consumes the scanner.

        ``strict_reference`` is accepted for callers written against the first rounds of this package (where the
        reference's walk was opt-in) and ignored with a DeprecationWarning: the walk is the only behaviour of
        ``max()`` now; ``strict_reference=False`` callers want :meth:`max_valid`.

        The u8 DiscreteMatrix scores steer which cells are looked at: starting from the best pending hit
        (or none) and the level ``dm.scale(threshold)``, cells are visited block by block in row-major
        order; a cell whose u8 score reaches the current level is re-scored in f32 and replaces the best
        hit when its score is greater, or equal at a greater position (scan.rs:237) -- and the level
        becomes ITS u8 score.  Consequences the reference has and this keeps: (a) positions are not
        tested against ``position + M <= L``; (b) while no hit is held the first candidate is accepted
        even if its f32 score is below the threshold; (c) a better cell whose u8 score lies under the
        level (the u8 score of the current best, an over-estimate) is skipped (scan.rs:227-243).
        ``saturate``: the u8 adds of the x86-64 ``dispatch`` pipeline (avx2.rs:336); ``False`` =
        Generic's wrapping adds.  :meth:`max_valid` is the variant without those corner cases."""
        if strict_reference is not None:
            import warnings
            warnings.warn("Scanner.max(strict_reference=...) is deprecated: max() always walks like the reference "
                          "(scan.rs:200-249); use max_valid() for the greatest valid hit", DeprecationWarning, stacklevel=2)
        return self._max_device(saturate)

    def _pending_state(self):
        """The reference scanner's state after the ``next()`` calls made so far (scan.rs:169-198): ``row`` = the
        block after the one the last yielded hit came from, ``hits`` = the not yet yielded hits of that block --
        derived from the complete hit list: (best pending hit or None, first row of the walk)."""
        thr = np.float32(self.threshold)
        rows, bs = self._seq.rows, self.block_size
        best: Optional[Tuple[int, np.float32]] = None
        first_block = 0
        if self._order is not None and self._next > 0:
            last = self._order[self._next - 1]
            blk = (int(self._positions[last]) % rows) // bs
            first_block = blk + 1
            rest = self._order[self._next:]
            rest = rest[(self._positions[rest] % rows) // bs == blk]
            for i in rest[::-1]:                       # the vector's order = reverse of the yield order
                sc = np.float32(self._scores[i])       # scan.rs:207-210; max_by keeps the LAST of equals
                if sc >= thr and (best is None or not (sc < best[1])):
                    best = (int(self._positions[i]), sc)
        self._order = np.zeros(0, np.int64)            # consumed (scan.rs:200 takes `self`)
        self._positions, self._scores, self._next = np.zeros(0, np.int64), np.zeros(0, np.float32), 0
        return best, first_block * bs

    def _max_device(self, saturate: bool) -> Optional[Hit]:
        """scan.rs:200-249 through ``lm_hip_scan_max_f32``: the walk itself runs on the device (csrc/scanmax.hip)."""
        pli, seq, pssm = self._seq._pli, self._seq, self._pssm
        best, first_row = self._pending_state()
        if seq.rows == 0 or len(seq) < len(pssm):
            return None if best is None else Hit(best[0], float(best[1]))
        dm = pssm.to_discrete()
        level = dm.scale(float(best[1])) if best is not None else dm.scale(float(np.float32(self.threshold)))
        w = np.ascontiguousarray(dm.data, dtype=np.uint8)
        found, hit = C.c_int(0), _ffi.Hit()
        st = pli._L.lm_hip_scan_max_f32(pli._h, pssm._device(pli), seq._h, w.ctypes.data, w.shape[1], int(bool(saturate)),
                                        int(level), int(best is not None), 0 if best is None else best[0],
                                        0.0 if best is None else float(best[1]), first_row, C.byref(found), C.byref(hit))
        if st == _ffi.ERR_BAD_ARGS and "leaves the striped matrix" in _ffi.last_error():
            raise IndexError("Scanner.max: " + _ffi.last_error())   # seq[pos + j] past the matrix: the reference panics
        check(st)
        return Hit(int(hit.position), float(hit.score)) if found.value else None

    def max_valid(self) -> Optional[Hit]:
        """NOT the reference's ``max()``: the best VALID hit not yet yielded -- ``score >= threshold``
        and ``position + M <= L`` like every hit ``__next__`` yields (scan.rs:186-189); greater score
        wins, equal scores go to the greater position.  Consumes the scanner.  On a fresh scanner the
        hit list is never built (a low threshold would select most of the sequence): the fused argmax
        gives the greatest score S of the matrix, and one scan at max(threshold, S) returns the few
        valid positions that reach it.  Differs from :meth:`max` exactly in that method's (a)-(c)."""
        if self._order is None:
            pli = self._seq._pli
            top = pli.score_argmax(self._pssm, self._seq)
            if top is None:
                self._order = np.zeros(0, np.int64)
                return None
            s_max = top[1]
            if s_max == s_max and s_max >= self.threshold:
                pos, sc = self._scan(s_max)
                if sc.size:  # valid positions (position + M <= L) that reach the matrix maximum
                    self._order = np.zeros(0, np.int64)
                    self._positions, self._scores = pos[:0], sc[:0]
                    return self._best(pos, sc)
                # the maximum sits in the padded tail only (finite weights for N): full list
            elif s_max == s_max:
                self._order = np.zeros(0, np.int64)  # nothing reaches the threshold
                self._positions, self._scores = np.zeros(0, np.int64), np.zeros(0, np.float32)
                return None
            self._collect()
        rest = self._order[self._next:]
        self._next = self._order.size
        return self._best(self._positions[rest], self._scores[rest])


# --- module-level helpers (lib.rs:1335-1451) ---------------------------------------------------


class Motif:
    def __init__(self, counts: Optional[CountMatrix], pwm: WeightMatrix, pssm: ScoringMatrix,
                 name: Optional[str] = None):
        self.counts, self.pwm, self.pssm, self.name = counts, pwm, pssm, name

    @property
    def protein(self) -> bool:
        return self.pssm.protein


def create(sequences: Iterable[str], *, protein: bool = False, name: Optional[str] = None) -> Motif:
    """lib.rs:1352-1386: counts -> to_freq(0.0).to_weight(None) -> to_scoring()."""
    encoded = [EncodedSequence(s, protein=protein) for s in sequences]
    counts = CountMatrix.from_sequences(encoded, protein=protein)
    pwm = counts.normalize(0.0)
    return Motif(counts, pwm, pwm.log_odds(), name)


def fasta_names(data, spans: np.ndarray) -> List[str]:
    """The record names behind the ``header_spans`` of ``Pipeline.stripe_fasta_set(data)``: the header up to its first
    whitespace, ``""`` for a bare ``>`` (the rule of ``scan_cli.read_fasta``; the ``\\r`` of a ``\\r\\n`` line end goes with
    the whitespace)."""
    view = memoryview(data).cast("B") if not isinstance(data, np.ndarray) else memoryview(np.ascontiguousarray(data, dtype=np.uint8))
    names = []
    for begin, end in np.asarray(spans, dtype=np.uint64).reshape(-1, 2).tolist():
        head = bytes(view[begin:end]).split(None, 1)
        names.append(head[0].decode("utf-8", "replace") if head else "")
    return names


def pack_2bit(encoded: np.ndarray, runs: bool = False):
    """Symbol bytes of a DNA sequence (A0 C1 T2 G3 N4, abc.rs:115-135) -> ``(packed, n)`` as
    ``Pipeline.stripe_2bit`` takes them: base i in bits 2*(i%4).. of byte i//4; N positions are packed as A and
    described by ``n`` -- a bit mask (bit i%8 of byte i//8; default) or, with ``runs=True``, an ``(k, 2)`` uint64
    array of ``(start, size)`` runs like a .2bit file's N blocks; ``None`` when the sequence has no N."""
    enc = np.ascontiguousarray(encoded, dtype=np.uint8)
    n = enc.size
    is_n = enc > 3
    two = np.where(is_n, 0, enc).astype(np.uint8)
    pad = (-n) % 4
    if pad:
        two = np.concatenate([two, np.zeros(pad, np.uint8)])
    q = two.reshape(-1, 4)
    packed = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8)
    if not is_n.any():
        return packed, None
    if not runs:
        return packed, np.packbits(is_n, bitorder="little")
    edges = np.flatnonzero(np.diff(np.concatenate([[0], is_n.view(np.int8), [0]])))
    return packed, np.stack([edges[0::2], edges[1::2] - edges[0::2]], axis=1).astype(np.uint64)


def stripe(sequence: str, *, protein: bool = False) -> StripedSequence:
    """lib.rs:1402-1409"""
    return EncodedSequence(sequence, protein=protein).stripe()


def scan(pssm: ScoringMatrix, sequence: StripedSequence, *, threshold: float = 0.0,
         block_size: int = 256) -> Scanner:
    """lib.rs:1437-1451.  The reference's Python ``scan()`` is DNA-only (its PyO3 class is
    instantiated for ``Dna``); the Rust ``Scanner`` is alphabet-generic (scan.rs:96-136), and so
    is the ``Scanner`` class here -- this module-level helper keeps the binding's restriction."""
    if pssm.protein or sequence.protein:
        raise ValueError("scanner only supports DNA")  # lib.rs scan()
    return Scanner(pssm, sequence, threshold, block_size)
