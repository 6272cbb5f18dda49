"""Resident DME pipeline: the batched hot path with its buffers kept in HBM.

    p = DMEPipeline(n, d, bits_per_dimension=1, torch_threads=1)
    est = p.step(x, X, n_div)        # K1 L1 (AS:624) -> K2 quantize (AS:625-640, writes q and
                                     # type codes) -> K3c client-ordered mean (ND:137-138)
    p.q, p.codes, p.l1, p.kmax       # the step's per-client outputs (overwritten by the next step)

Pipelines (what K2 writes and what the mean reads; est has the same bits in all three):
    "codes"   q and the int8 type codes; the mean reads the codes (1 B per coordinate), and a
              client whose counts overflowed its codes (kmax > 127) is read from q instead
              (uq_codes_q_mean_f32), so est is always the client-ordered mean of q
    "q"       q only; the mean reads q (4 B per coordinate) -- the drop-in's output form
    "encode"  codes only (no q); the mean reads the codes.  An overflowed client cannot be
              recovered without q: check_status() raises OverflowError for it.
    "codes4"  q and the type codes as 4-bit fields (p.nib, uint8 [n, d/2]: the int8 code's low
              nibble, exact for counts <= 7 -- every client at R <= 2 but for extreme tails);
              the mean reads the nibbles (0.5 B per coordinate) and a client with kmax > 7
              from q (uq_nibbles_q_mean_ld_f32).  n >= 256 and d % 4096 == 0 (stream form).
              `codes4_fits(n, d, bits)` says when it applies; the bench's default.

Output placement.  K2 writes q (4*d B per client) and the int8 codes (1*d) while reading x.
On MI355X its time depends on where the OUTPUT buffers land in physical memory: with x fixed
and q + codes re-allocated ten times in one process K2 took 1.66-2.03 ms on the C2 batch, with
q + codes fixed and x re-allocated ten times 1.67-1.73 ms (profiles/r02d_exp_placement_split.jsonl);
the code layout does not matter (tile-major codes follow the same modes,
profiles/r02c_exp_codes_layout.jsonl).  The pipeline's outputs are long-lived, so
`probe_outputs` allocates candidate (q, codes) sets (each on its own pages, all held until
the choice: freeing a loser would hand its pages to the next candidate), times K2 on each
with the real batch until it has seen both speeds, keeps the fastest and frees the rest: a
one-time calibration like a workspace autotune.  Results do not depend on the buffers
chosen.  Only callers that keep a pipeline resident get the probed speed; the one-shot
batched APIs (quantize_dequantize, quantize_mean, ...) allocate per call and land in either
mode.

Every launch goes through the C-ABI (include/uq_dme.h); nothing here computes on the CPU."""
from __future__ import annotations

import statistics

import torch

from . import _lib, _runtime
from ._runtime import ptr
from .rates import RATE_TABLE, rate_to_m

__all__ = ["DMEPipeline", "PIPELINES", "codes4_fits"]

PIPELINES = ("codes", "q", "encode", "codes4")


def _codes4_shape(n: int, d: int) -> bool:
    """The stream form's shape rule: n >= 256 and d a multiple of 4096, at most 2^29."""
    return n >= 256 and d % 4096 == 0 and d <= (1 << 29)


def codes4_fits(n: int, d: int, bits_per_dimension=1) -> bool:
    """The 4-bit code pipeline's shape conditions, and a rate whose counts stay <= 7 for
    Gaussian-like clients (m <= 0.64 d: R <= 2)."""
    return _codes4_shape(n, d) and RATE_TABLE.get(bits_per_dimension, 1e9) <= 0.64


class DMEPipeline:
    def __init__(self, n: int, d: int, bits_per_dimension=1, *, m: int | None = None, torch_threads: int = 1,
                 pipeline: str = "codes", device=None):
        current = _runtime.device()                     # raises without a GPU
        if pipeline not in PIPELINES:
            raise ValueError(f"pipeline must be one of {PIPELINES}")
        if pipeline == "codes4" and not _codes4_shape(n, d):
            raise ValueError("pipeline 'codes4' needs n >= 256 and d a multiple of 4096 (<= 2^29)")
        self.dev = current if device is None else torch.device(device)
        self.n, self.d = int(n), int(d)
        self.m = int(m) if m is not None else rate_to_m(bits_per_dimension, d)
        self.T = int(torch_threads)
        self.pipeline = pipeline
        self.lib = _lib.load()
        self.ws_bytes = _runtime.workspace_bytes("uq_workspace_bytes", self.n, self.d, self.T)
        self.ws = torch.zeros(max(self.ws_bytes, 1 << 16), dtype=torch.uint8, device=self.dev)
        self.l1 = torch.empty(self.n, dtype=torch.float32, device=self.dev)
        self.kmax = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        self.est = torch.empty(self.d, dtype=torch.float32, device=self.dev)
        self.codes = self.nib = None
        self.q, c = self._alloc_outputs()
        self._set_codes(c)
        self.probe_report = None
        self._codes_valid = False       # the last K2 launch wrote codes (and kmax)
        self._nib_valid = False         # ... as 4-bit fields
        self._mean_without_q = False    # the last mean read codes with no q to fall back to

    @property
    def write_q(self) -> bool:
        return self.pipeline != "encode"

    # ---- buffers ---------------------------------------------------------------------
    def _alloc_codes(self, pipeline):
        if pipeline == "codes4":
            return torch.empty((self.n, self.d // 2), dtype=torch.uint8, device=self.dev)
        return torch.empty((self.n, self.d), dtype=torch.int8, device=self.dev) if pipeline != "q" else None

    def _alloc_outputs(self):
        q = torch.empty((self.n, self.d), dtype=torch.float32, device=self.dev) if self.write_q else None
        return q, self._alloc_codes(self.pipeline)

    def _set_codes(self, c):
        if self.pipeline == "codes4":
            self.nib = c
        else:
            self.codes = c

    def _codes_for(self, pl):
        """The code buffer a launch of pipeline `pl` uses (int8 codes or 4-bit fields), made on
        first use when a step overrides the pipeline's own kind."""
        if pl == "codes4":
            if self.nib is None:
                self.nib = self._alloc_codes("codes4")
            return self.nib
        if self.codes is None:
            self.codes = self._alloc_codes("codes")
        return self.codes

    @staticmethod
    def _ld(t) -> int:
        """Row pitch of an output buffer (the launches take pitched rows, e.g. a caller's views)."""
        return int(t.stride(0)) if t is not None and t.dim() == 2 and t.shape[0] > 1 else (0 if t is None else t.shape[-1])

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    # ---- the three launches ----------------------------------------------------------
    def l1_norms(self, x):
        _lib.check(self.lib.uq_l1_torch_order_f32(ptr(x), self.n, self.d, self.T, ptr(self.l1), ptr(self.ws),
                                                  self.ws_bytes, self._stream()), "uq_l1_torch_order_f32")

    def quantize(self, x, X, q=None, codes=None, pipeline: str | None = None):
        """K2 with the batch's L1 (l1_norms first).  `pipeline` overrides what is written for
        this launch ("q": q only, "encode": codes only, "codes": both)."""
        pl = pipeline or self.pipeline
        q = (self.q if q is None else q) if pl != "encode" else None
        if pl != "encode" and q is None:
            raise ValueError("this pipeline holds no q buffer")
        if pl == "codes4":
            nib = self._codes_for(pl) if codes is None else codes
            _lib.check(self.lib.uq_type_unbiased_nibbles_ld_f32(ptr(x), ptr(q), max(self._ld(q), self.d), ptr(nib),
                                                                max(self._ld(nib), self.d // 2), ptr(self.kmax), self.n,
                                                                self.d, self.m, ptr(X), ptr(self.l1), None, self.T,
                                                                ptr(self.ws), self.ws_bytes, self._stream()),
                       "uq_type_unbiased_nibbles_ld_f32")
            self._codes_valid = True
            self._nib_valid = True
            return
        self._nib_valid = False
        codes = (self._codes_for(pl) if codes is None else codes) if pl != "q" else None
        _lib.check(self.lib.uq_type_unbiased_codes_ld_f32(ptr(x), ptr(q), max(self._ld(q), self.d), ptr(codes),
                                                          max(self._ld(codes), self.d),
                                                          ptr(self.kmax if codes is not None else None), self.n, self.d,
                                                          self.m, ptr(X), ptr(self.l1), None, self.T, ptr(self.ws),
                                                          self.ws_bytes, self._stream()),
                   "uq_type_unbiased_codes_ld_f32")
        self._codes_valid = codes is not None

    def mean(self, n_div: float, accumulate: bool = False, est=None, pipeline: str | None = None):
        """K3 (from q) or K3c (from the codes, overflowed clients from q when it was written)."""
        pl = pipeline or self.pipeline
        est = self.est if est is None else est
        if pl == "q":
            self._mean_without_q = False
            _lib.check(self.lib.uq_client_mean_f32(ptr(self.q), self.n, self.d, max(self._ld(self.q), self.d),
                                                   float(n_div), int(bool(accumulate)), ptr(est), self._stream()),
                       "uq_client_mean_f32")
        elif pl == "codes4":
            self._mean_without_q = False
            _lib.check(self.lib.uq_nibbles_q_mean_ld_f32(ptr(self.nib), max(self._ld(self.nib), self.d // 2),
                                                         ptr(self.q), max(self._ld(self.q), self.d), ptr(self.l1),
                                                         ptr(self.kmax), self.n, self.d, self.m, float(n_div),
                                                         int(bool(accumulate)), ptr(est), self._stream()),
                       "uq_nibbles_q_mean_ld_f32")
        else:
            q = self.q if pl == "codes" else None
            self._mean_without_q = q is None
            _lib.check(self.lib.uq_codes_q_mean_ld_f32(ptr(self.codes), max(self._ld(self.codes), self.d), ptr(q),
                                                       max(self._ld(q), self.d), ptr(self.l1), ptr(self.kmax), self.n,
                                                       self.d, self.m, float(n_div), int(bool(accumulate)), ptr(est),
                                                       self._stream()), "uq_codes_q_mean_ld_f32")
        return est

    def step(self, x, X, n_div=None, accumulate: bool = False, *, est=None, events=None,
             pipeline: str | None = None, mean: bool = True):
        """One pass of the hot path over the resident batch x[n, d] (f32, contiguous, on the
        device) with per-client uniforms X[n] (device f32).  Returns est (+)= sum_j q_j / n_div
        (into `est` when given, else the pipeline's own buffer).  `events`: four HIP events
        recorded on the stream before K1, after K1, after K2 and after the mean.  mean=False
        stops after K2 (a caller folding q itself, e.g. ShardedDME's ordered chain)."""
        self._check(x, X)
        ev = events or (None, None, None, None)
        if ev[0] is not None:
            ev[0].record()
        self.l1_norms(x)
        if ev[1] is not None:
            ev[1].record()
        self.quantize(x, X, pipeline=pipeline)
        if ev[2] is not None:
            ev[2].record()
        out = self.mean(self.n if n_div is None else n_div, accumulate, est=est, pipeline=pipeline) if mean else None
        if ev[3] is not None:
            ev[3].record()
        return out

    def _check(self, x, X):
        if x.shape != (self.n, self.d) or x.dtype != torch.float32 or not x.is_contiguous() or x.device != self.dev:
            raise ValueError(f"x must be a contiguous f32 [{self.n}, {self.d}] tensor on {self.dev}")
        if X.numel() != self.n or X.dtype != torch.float32 or X.device != self.dev:
            raise ValueError("X must hold one f32 draw per client on the device")

    # ---- output placement ------------------------------------------------------------
    def probe_outputs(self, x, X, candidates: int = 16, reps: int = 3, batch: int = 4, spread: float = 1.15,
                      min_candidates: int = 1, reserve_frac: float = 0.25):
        """Time K2 on output sets (the current one included), keep the fastest.  Sets are
        added `batch` at a time, up to `candidates`, until the probe has seen both speeds
        (slowest / fastest >= `spread`; the fast and slow modes are 15-20 % apart, and
        spread 1.10 once stopped on an intermediate 1.74 ms set against 1.92-1.98 ms ones,
        profiles/r04a_bench.json): with ~30-60 % of sets fast, six fixed candidates left
        ~1 rank in 8 without a fast set.  No set is added once free device memory would
        drop below `reserve_frac` of the device (the held sets are the probe's only cost:
        ~5 GB each at 1024 x 2^20).  Needs the batch's L1 (runs K1 first).  Returns the
        report: ms per candidate, the chosen one, and the median over all candidates (what a
        caller allocating fresh outputs gets on average)."""
        self._check(x, X)
        self.l1_norms(x)
        sets, times = [(self.q, self.nib if self.pipeline == "codes4" else self.codes)], []
        code_bytes = {"q": 0.0, "codes4": 0.5}.get(self.pipeline, 1.0)
        set_bytes = int(self.n * self.d * ((4 if self.write_q else 0) + code_bytes))

        def time_set(q, c):
            for _ in range(2):
                self.quantize(x, X, q, c)
            torch.cuda.synchronize(self.dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                self.quantize(x, X, q, c)
            e1.record()
            torch.cuda.synchronize(self.dev)
            return e0.elapsed_time(e1) / reps

        def room() -> bool:
            free, total = torch.cuda.mem_get_info(self.dev)
            return free - set_bytes >= reserve_frac * total

        times.append(time_set(*sets[0]))
        capped = False
        while len(sets) < candidates and (len(sets) < min_candidates or max(times) < spread * min(times)):
            for _ in range(min(batch, candidates - len(sets))):
                if not room():
                    capped = True
                    break
                sets.append(self._alloc_outputs())
                times.append(time_set(*sets[-1]))
            if capped:
                break
        best = min(range(len(sets)), key=lambda i: times[i])
        self.q, c = sets[best]
        self._set_codes(c)
        del sets
        torch.cuda.empty_cache()
        self.probe_report = {"candidates": len(times), "k2_ms": [round(t, 4) for t in times], "chosen": best,
                             "k2_ms_chosen": round(times[best], 4),
                             "k2_ms_median_unprobed": round(statistics.median(times), 4),
                             "memory_capped": capped}
        return self.probe_report

    def overflowed(self) -> int:
        """Clients of the last step whose counts overflowed their codes (int8: > 127; 4-bit:
        > 7, read from q by the mean) (synchronises)."""
        if not self._codes_valid:
            return 0
        return int(torch.count_nonzero(self.kmax > (7 if self._nib_valid else 127)).item())

    def check_status(self):
        """Synchronise; raise if an in-kernel wait timed out, or if the last mean was taken
        from codes alone (pipeline "encode", or a step overridden to it) while a client's
        codes overflowed, since its est contribution is then wrong."""
        _lib.check(self.lib.uq_check_status(ptr(self.ws), self._stream()), "uq_check_status")
        if self._mean_without_q and self.overflowed():
            raise OverflowError("type codes overflowed (lattice counts > 127) in an encode-only step: "
                                "est is wrong for those clients; use pipeline='codes' (falls back to q)")
