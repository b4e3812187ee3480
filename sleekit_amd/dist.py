"""Row-sharded quantization of a stream of layers over the GPUs of one node.

Given the shared factor U, every output row of W goes through the loop, the local search
and the error on its own (sleekit/obq.py:106-137, 264-346, 89-95 have no cross-row term),
so the path shards by rows with no data-path collective.  What does NOT shard is the
n x n factorisation; over a stream of layers it is spread instead: rank (l mod G) factors
layer l and its packed factor (status, order, upper triangle of U) crosses xGMI exactly once,
while every rank runs rows [r R/G, (r+1) R/G) of every layer.

One process per GPU; `torch.distributed` must be initialised by the caller (backend "nccl"
is RCCL on ROCm).  The exchange is one asynchronous all-gather per round of G layers (G
simultaneous broadcasts, one root each), issued up front so the loops of round g overlap the
factorisations and the transfer of round g+1; on a single rank nothing is communicated.

The module is engine-agnostic: `backend` supplies factorize / run_rows (class Backend below is the whole contract, with
every optional hook's default), which lets the CPU test-suite drive the same scheduling code over gloo with a stand-in backend.
"""

import collections
import contextlib
import ctypes
import operator
import os
import types

import torch
import torch.distributed as dist


# Test hook: exchange (pack, all-gather, unpack) even on a single rank, so that a one-GPU box can drive the
# RCCL path end to end (tests/test_gpu_parity.py::test_exchange_over_rccl_single_rank).
always_exchange = False


# Measurement hook (tools/micro_rank_of_n.py): (rank, size) makes this process behave as ONE rank of a larger job on a
# single GPU -- same rounds, roots, streams and kernels -- with the all-gather replaced by a local hand-over of this
# rank's own payload in every slot (the results are meaningless, the work is that of the real rank).
rehearse = None
_rehearsal_payloads = {}
_stream_pool = {}  # device index -> the side streams every HipBackend of this process hands out (HipBackend.streams)


class _Done:
    """Stands in for the work handle of a collective: wait() orders the current stream behind `event`."""

    def __init__(self, event=None):
        self.event = event

    def wait(self):
        if self.event is not None:
            torch.cuda.current_stream().wait_event(self.event)
        return True


def world():
    if rehearse is not None:
        return rehearse
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def row_range(R, rank, size):
    """Rows [lo, hi) of rank `rank`: contiguous, sizes differ by at most one, covers [0, R) exactly."""
    base, extra = divmod(R, size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def factor_root(position, size):
    """Root of the layer at `position` of the processing order (plan_rounds): positions go round the ranks."""
    return position % size


def _layer_kind(layer):
    """What a layer's scales make of its loop: "unscaled", "row" (one scale per row, `scale`) or ("group", g) (one per row
    and per group of g columns, `gscale` / `group_size`).  Every bucketing decision -- rounds, short rounds, groups of
    rounds, loop batches -- keys on (shape, kind): layers of different kinds never share a loop."""
    if layer.get("gscale") is not None:
        return ("group", int(layer["group_size"]))
    return "row" if layer.get("scale") is not None else "unscaled"


def check_layers(layers, moves=0):
    """The group-scale keys of a stream, checked before anything runs -- on every rank alike, since every rank holds every
    layer's inputs -- so that a refusal leaves no rank waiting in a collective.  `gscale` (R, n / group_size) float32 and
    `group_size` (an int that divides n) come together and exclude `scale`.  Grouped layers have no local search
    (NotImplementedError when moves > 0).  Group offsets (`goffset`) are not supported in the stream: NotImplementedError."""
    grouped = False
    for l, lay in enumerate(layers):
        if "goffset" in lay:
            raise NotImplementedError(f"layer {l}: group offsets (`goffset`) are not supported in quantize_stream")
        S, g = lay.get("gscale"), lay.get("group_size")
        if S is None and g is None:
            continue
        R, n = lay["W"].shape
        if S is None or g is None:
            raise ValueError(f"layer {l}: group scales need both `gscale` and `group_size`")
        if lay.get("scale") is not None:
            raise ValueError(f"layer {l}: `gscale` and `scale` are exclusive (one scale per row, or per row and group)")
        try:
            g = operator.index(g) if not isinstance(g, bool) else 0
        except TypeError:
            g = 0
        if g < 1 or n % g != 0:
            raise ValueError(f"layer {l}: group_size must be an int >= 1 that divides the {n} columns (got {lay['group_size']!r})")
        if tuple(S.shape) != (R, n // g) or S.dtype != torch.float32:
            raise ValueError(f"layer {l}: gscale must be float32 ({R}, {n // g}) for a ({R}, {n}) layer with group_size {g}; "
                             f"got {S.dtype} {tuple(S.shape)}")
        grouped = True
    if grouped and moves > 0:
        raise NotImplementedError("quantize_stream: local search (nb_ls_moves > 0) is not available with group scales")


def plan_rounds(layers, size, bucket=True):
    """Rounds of at most `size` layers, each of ONE shape, and every layer's factor root.

    A model's layers come in an order that mixes shapes (an OPT / BLOOM block is {d x d ..., 4d x d, d x 4d};
    reference: experiments/compare.py:37-53 walks one directory per layer), but they are independent
    (compare.py:50-131), so the stream is bucketed by (rows, columns, _layer_kind) and each bucket cut into rounds: the
    row shards of a round's layers then go through the kernels as one batch (HipBackend.run_round).  Roots follow
    the position in this processing order, so a bucket's partial last round does not leave the same ranks idle
    every time.  Returns (rounds, root): rounds = lists of layer indices, root[l] = the rank that factors layer l.
    """
    n_layers = len(layers)
    if size <= 1 or not bucket:
        groups = [list(range(n_layers))]
    else:
        by_shape = {}
        for l, lay in enumerate(layers):
            key = (tuple(lay["W"].shape), tuple(lay["H"].shape), _layer_kind(lay))
            by_shape.setdefault(key, []).append(l)
        groups = list(by_shape.values())  # in order of first appearance
    rounds, root, position = [], [None] * n_layers, 0
    for members in groups:
        for i in range(0, len(members), max(size, 1)):
            chunk = members[i:i + max(size, 1)]
            for l in chunk:
                root[l] = factor_root(position, max(size, 1))
                position += 1
            rounds.append(chunk)
    return rounds, root


class Backend:
    """What quantize_stream asks of an engine.  Required: payload_words(n), alloc_payload(words, device), pack(factor, words),
    unpack(payload, n), factorize(layer), run_rows(layer, lo, hi, factor).  Everything optional is below with the default the
    scheduler sees -- it probes nothing, and looks every method up on the instance at call time (tests put counters there).
    The defaults are the plainest schedule: in order on the caller's stream, a layer per factorisation, a layer per loop."""

    moves = 0                        # local-search moves (check_layers: none with group scales)
    exchange_log = None              # a list: every all-gather is timed between two events and appended (measurement)
    bucket_by_shape = True           # several ranks: rounds of one shape (plan_rounds)
    rounds_on_factor_streams = True  # a batched round runs on the stream that factored this rank's layer of it
    factor_chains = False            # factorize_many is ONE launch chain: a rank's layers of a group of rounds form one job on
    #                                  one stream (up to _chain_cap of them), not a job each on rotating streams
    group_bytes = 1 << 32            # bytes the factorisations of one chain may hold (_chain_cap)
    local_batch = 1                  # one rank: small layers per batched round (run_round_local); also caps a short round
    short_rows = 4096                # one rank: stacked rows of a round of short-wide layers (_short_rounds) ...
    short_factor_batch = 1           # ... and how many of its factorisations share a chain
    tall_stack = 1                   # one rank: full-height layers per loop (run_tall)
    _factor_rotation = _loop_rotation = 0  # where the rotation over the factor / loop streams stands (_Lanes)

    def streams(self):  # (factor streams, comm stream, loop streams), or no side streams
        return None, None, None

    def group_limit(self, layer, rows):  # layers of this shape, `rows` per rank, in one loop batch (0: round by round)
        return 0

    def can_batch(self, round_layers, lo, hi):  # run_round(round_layers, lo, hi, payloads) takes these shards as one batch
        return False

    def wants_local_batch(self, layer):  # one rank: in rounds of its shape through run_round_local(round_layers)
        return False

    def wants_stacked_loop(self, layer):  # one rank: factored in chains, looped by run_round_stacked(round_layers, factors)
        return False

    def wants_tall_stack(self, layer):  # one rank: its loop shares launches with its neighbours', run_tall(stack_layers, factors)
        return False

    def factorize_many(self, layers):
        return [self.factorize(lay) for lay in layers]

    def note_statuses(self, infos, layers, defer=False):  # every layer's factorisation status word, once per call
        pass


class HipBackend(Backend):
    """The real thing: sleekit_amd.engine on the current device."""

    factor_chains = True

    def __init__(self, quantizer, act_order="diag", damp=0.01, nb_ls_moves=0, with_error=True, overlap=True):
        from . import engine

        self.engine, self.quantizer, self.overlap = engine, quantizer, overlap
        self.act_order, self.damp, self.moves, self.with_error = act_order, damp, nb_ls_moves, with_error
        for knob in ("local_batch", "local_batch_cols", "group_rows", "short_factor_batch", "short_rows", "tall_stack", "group_wide_rows",
                     "group_bytes"):  # (measurement knobs: SLK_LOCAL_BATCH ...)
            setattr(self, knob, int(os.environ.get("SLK_" + knob.upper(), getattr(self, knob))))

    def streams(self):
        """(factor streams, comm stream, loop streams), created once; (None, None, None) = everything in order."""
        if not self.overlap:
            return None, None, None
        if not hasattr(self, "_streams"):
            nf, nl = (self.overlap if isinstance(self.overlap, tuple) else (3, 1))  # best on 8 hardware queues
            # ONE set of side streams per device and process, shared by every backend: the first streams a process makes --
            # as many as it has hardware queues, the default stream included -- have a queue each, later ones double up
            # with them and stop overlapping.  A second backend with streams of its own
            # ran like a different program (bench.py: OPT-350M 69.8 ms per step after the headline's backend, 61.2 on its streams).
            dev_index = torch.cuda.current_device()
            pool = _stream_pool.setdefault(dev_index, [])
            while len(pool) < nf + nl + 1:
                pool.append(torch.cuda.Stream())
            self._streams = (pool[:nf], pool[nf], pool[nf + 1:nf + 1 + nl])
        return self._streams

    def payload_words(self, n):
        """slk_factor_pack's words, plus one: whether H is bit-wise symmetric (the root checks it once for all ranks)."""
        from . import _lib

        return int(_lib.lib.slk_factor_payload_words(n)) + 1

    def alloc_payload(self, words, device):
        return torch.empty(words, dtype=torch.int64, device=device)

    def pack(self, factor, words):
        """(order, U, info) -> the first payload_words(n) of a `words`-long int64 buffer:
        status, order, packed upper triangle of U."""
        from . import _device as dev
        from . import _lib

        order, U, info = factor[:3]
        n = U.shape[0]
        payload = self.alloc_payload(words, U.device)
        _lib.check(_lib.lib.slk_factor_pack(dev.ptr(U), dev.ptr(order), dev.ptr(info), n, dev.ptr(payload), dev.stream_handle()))
        mark = self.payload_words(n) - 1
        if len(factor) > 3:
            payload[mark:mark + 1].copy_(factor[3])  # int32 -> int64 on the way
        else:
            payload[mark:mark + 1].fill_(-1)  # not checked by the root
        return payload

    def unpack(self, payload, n):
        from . import _device as dev
        from . import _lib

        order = torch.empty(n, dtype=torch.int64, device=payload.device)
        U = torch.empty((n, n), dtype=torch.float64, device=payload.device)
        info = torch.empty(1, dtype=torch.int32, device=payload.device)
        _lib.check(_lib.lib.slk_factor_unpack(dev.ptr(payload), n, dev.ptr(U), dev.ptr(order), dev.ptr(info), dev.stream_handle()))
        mark = self.payload_words(n) - 1
        return order, U, info, payload[mark:mark + 1].to(torch.int32)  # + the root's symmetry verdict (-1: none)

    def factorize(self, layer):
        eng = self.engine
        H, n = layer["H"], layer["H"].shape[0]
        # (err / sqerr keys need the statistics of ALL rows, before sharding)
        miss = eng.sort_keys(layer["W"], H, eng.require_uniform(self.quantizer), self.act_order, self.damp, scale=layer.get("scale"),
                             gscale=layer.get("gscale"), group_size=layer.get("group_size"))
        factor = eng.factorize(H, n, self.damp, eng.order_mode_code(self.act_order), miss)
        if self.with_error:  # the layer error wants to know whether H is symmetric: decided here, once per layer
            factor = factor + (self._symmetry(layer),)
        return factor

    def _plain_order(self):
        """none / diag: the orders whose keys come from H alone, inside the factorisation -- what a batched one can make."""
        from . import _lib

        return self.engine.order_mode_code(self.act_order) in (_lib.ORDER_NONE, _lib.ORDER_DIAG)

    def _symmetry(self, layer):
        """int32[1] on the device: 1 iff H is bit-wise symmetric.  A layer dict may VOUCH for it (`symmetric=True`: the caller
        has checked, e.g. once when the statistics were loaded): no check per call then, and the layer's error can be the one
        the loop or the search carries instead of a product of its own (see run_rows, _run_stacked)."""
        if layer.get("symmetric") is True:
            dev_ = layer["H"].device
            if getattr(self, "_yes", None) is None or self._yes.device != dev_:
                self._yes = torch.ones(1, dtype=torch.int32, device=dev_)
            return self._yes
        return self.engine.symmetry_flag(layer["H"])

    def factorize_many(self, layers):
        """The factors of several layers of ONE width in launches that cover them all (engine.factorize_batch: bit-equal to
        factorize, one by one): what a rank owes to a group of rounds of small layers."""
        eng = self.engine
        n = layers[0]["H"].shape[0]
        mode = eng.order_mode_code(self.act_order)
        if not self._plain_order() or any(lay["H"].shape[0] != n for lay in layers) or len(layers) > 64:
            return [self.factorize(lay) for lay in layers]
        order, U, info = eng.factorize_batch([lay["H"] for lay in layers], n, self.damp, mode)
        out = []
        for b, lay in enumerate(layers):
            fac = (order[b], U[b], info[b:b + 1])
            if self.with_error:
                fac = fac + (self._symmetry(lay),)
            out.append(fac)
        return out

    group_rows = 8192  # stacked (padded) rows a loop batch of small shards may reach
    group_bytes = 1 << 32  # ... and the bytes of their stacked factors (24 factors of 4096 columns)
    # WIDE layers join groups too when a rank's shard of them is this few rows (the 1024 x 4096 layers of OPT-350M /
    # BLOOM-560M from 4 ranks up): a rank then owes a group several 4096-column factorisations, and they share ONE launch
    # chain (factorize_many) instead of following one another round by round -- one rank of 8, rehearsed: OPT-350M 12.15 ->
    # 11.06 ms per step, BLOOM-560M 12.9 -> 11.4; one of 4 on OPT-350M 20.3 -> 17.0.
    group_wide_rows = 256
    # Wide layers of few rows on one rank (the 1024 x 4096 layers of OPT-350M / BLOOM-560M: a 4096-column factorisation
    # each, for a loop of 1024 rows) go in rounds of `short_rows` stacked rows, and a round's factorisations share ONE launch
    # chain (factorize_many): the chain of 72 narrow launches is what such a layer costs, and six matrices ride it as well
    # as one.  OPT-350M 59.5 -> 51.8 ms per step, BLOOM-560M 69.2 -> 61.6 (four per chain and 4096 rows: 52.7 / 62.3; two:
    # 56.5 / 65.7).  Full-height layers gain nothing from sharing a chain (headline 25.6 ms either way: the chip is full
    # of their wide kernels), 4096 x 11008 layers lose (506 -> 518).
    short_factor_batch = 8  # at most this many factorisations per launch chain (1: one by one, on rotating streams)
    short_rows = 6144

    def group_limit(self, layer, rows):
        """How many layers of this shape, `rows` of them on this rank, go through the loop as one batch (0: round by round).
        Small layers only: their shards are chains of short launches (wants_local_batch), and the stacked factors must fit."""
        if rows <= 0:
            return 0
        if not self.wants_local_batch(layer):
            # wide layers whose SHARDS are a few rows: a rank's factorisations of consecutive rounds in one chain (below)
            if not (self.group_wide_rows and rows <= self.group_wide_rows and self._plain_order()):
                return 0
        n = layer["H"].shape[0]
        padded = (rows + 127) // 128 * 128
        return int(min(64, self.group_rows // padded, self.group_bytes // (8 * n * n)))

    def note_statuses(self, infos, layers, defer=False):
        """The status words of the layers' factorisations (0, or 1 + the failing pivot), one per layer of the stream:
        LinAlgError like the reference's np.linalg.cholesky (sleekit/obq.py:49-50), naming the layer -- now (ONE read
        of all the words), or at _device.raise_pending() when deferred (the words may still be in flight on a side
        stream) or when _device.lazy_errors is set."""
        from . import _device as dev

        def label(l):
            R, n = layers[l]["W"].shape
            return f"quantize_stream: layer {l} ({R} x {n}), compute_hessian_chol"

        have = [l for l, info in enumerate(infos) if info is not None]
        if not have:
            return
        if defer or dev.lazy_errors:
            for l in have:
                dev.note_info(infos[l], label(l), defer=True)
            return
        codes = torch.cat([infos[l].reshape(1) for l in have]).cpu().tolist()
        for l, code in zip(have, codes):
            if code != 0:
                dev.raise_not_pd(code, label(l))

    def run_rows(self, layer, lo, hi, factor):
        eng = self.engine
        if hi <= lo:  # fewer rows than ranks: this rank holds none of this layer
            n, device = layer["W"].shape[1], layer["W"].device
            return dict(Q=torch.empty((0, n), dtype=torch.float32, device=device), idx=torch.empty((0, n), dtype=torch.uint8, device=device),
                        row_err=torch.empty(0, dtype=torch.float32, device=device) if self.with_error else None, rows=(lo, hi))

        def shard(key):
            return layer[key][lo:hi].contiguous() if layer.get(key) is not None else None

        W, sc, S = shard("W"), shard("scale"), shard("gscale")
        carried = self._carried_error([layer])
        # (lookahead = "alone on the GPU": with overlapping streams the loop takes the window kernel's least-chip-time form)
        res = eng.quantize_layer(W, layer["H"], self.quantizer, sc, self.act_order, self.damp, self.moves, *self.blocks,
                                 factor=factor[:3], lookahead=not self.overlap, want_ls_error=carried == "search",
                                 want_loop_error=carried == "loop", gscale=S, group_size=layer.get("group_size"))
        err = None
        if res.ls_error is not None:  # carried through the search (scaled domain: times scale^2)
            err = res.ls_error if sc is None else (res.ls_error * sc) * sc
        elif res.loop_error is not None:  # carried through the loop (of the de-scaled Q already)
            err = res.loop_error
        elif self.with_error and len(factor) > 3:  # the verdict on H's symmetry came with the factor
            err = eng.row_errors_batch(W[None], res.Q[None], [layer["H"]], factor[3])[0]
        elif self.with_error:
            err = eng.row_errors(W, res.Q, layer["H"])
        return dict(Q=res.Q, idx=res.idx, row_err=err, rows=(lo, hi))

    blocks = (32, 8)  # min_block_size, num_blocks of every loop of the stream

    def _carried_error(self, layers):
        """Where the error of these layers (of one kind) comes from without a product of its own: "search" or "loop" for
        Hessians the caller vouches to be symmetric (layer["symmetric"] is True) -- the search carries every row's error with it,
        and so does the loop (the factor is this H's at self.damp on every rank; not with group scales, and unless
        engine.loop_error_route() says no) -- else None: the product (engine.row_errors*)."""
        if not self.with_error or layers[0].get("gscale") is not None or not all(lay.get("symmetric") is True for lay in layers):
            return None
        if self.moves > 0:
            return "search"
        return "loop" if self.engine.loop_error_route() else None

    # -- a whole round at once: the row shards of the G layers of a round go through every kernel together
    min_batch = 2  # (tests set 1 to send single-layer rounds through run_round as well)

    def can_batch(self, round_layers, lo, hi):
        if len(round_layers) < self.min_batch or len(round_layers) > 64 or hi == lo:
            return False
        first = round_layers[0]
        kind = _layer_kind(first)
        return all(lay["W"].shape == first["W"].shape and lay["H"].shape == first["H"].shape
                   and _layer_kind(lay) == kind for lay in round_layers)

    def run_round(self, round_layers, lo, hi, payloads):
        """Shards of the round's layers from their packed factors: unpack into one stacked factor, ONE loop and
        ONE error evaluation over all the layers (engine.gptq_loop) -- R / G rows of a single layer leave
        most of the chip idle, the round's G shards together are a full layer's worth of rows."""
        from . import _device as dev
        from . import _lib

        B, n = len(round_layers), round_layers[0]["H"].shape[0]
        device = round_layers[0]["W"].device
        # the stacked factors live in a buffer per stream, zeroed once: only the upper triangles are rewritten each round
        # (use on one stream is ordered; rounds on other streams have buffers of their own)
        if not hasattr(self, "_ustacks"):
            self._ustacks = {}
        # (ONE buffer per stream and width, grown to the largest batch seen and sliced: a buffer per batch size pinned up to
        # 4 GiB for every distinct B, and a shorter last group added a second one)
        key = (device.index, dev.stream_handle(), n)
        U = self._ustacks.get(key)
        if U is None or U.shape[0] < B:
            U = self._ustacks[key] = torch.zeros((B, n, n), dtype=torch.float64, device=device)
        U = U[:B]
        order = torch.empty((B, n), dtype=torch.int64, device=device)
        info = torch.empty(B, dtype=torch.int32, device=device)
        # (every rank runs the same backend settings, so with_error here means the roots packed real verdicts)
        known = torch.empty(B, dtype=torch.int32, device=device) if self.with_error else None
        ptrs = (ctypes.c_void_p * B)(*[dev.ptr(p) for p in payloads])
        # one launch for the round's payloads (a launch per layer is bound by the number of launches: 16 us each)
        _lib.check(_lib.lib.slk_factor_unpack_upper_batch(ptrs, B, n, dev.ptr(U), dev.ptr(order), dev.ptr(info), dev.ptr(known),
                                                          dev.stream_handle()))
        return self._run_stacked(round_layers, lo, hi, order, U, info, known)

    # -- one rank, small layers: a round of same-shaped layers is factored AND looped in launches that cover them all
    local_batch = 8          # layers per such round (1: off)
    local_batch_cols = 1536  # widest layer that takes this route whatever its rows (up to twice that with <= 1024 rows)

    def wants_local_batch(self, layer):
        """Small layers are bound by the host's launch rate (a 768-column layer is ~50 launches of microseconds each):
        batched by shape, a round of them costs the launches of one (OPT-125M, 72 layers: 47.8 -> 17.6 ms; rounds of 16
        or 4096-column layers in them changed nothing).  Big layers fill the chip alone and overlap better on separate
        streams (factor chains beside loops)."""
        R, n = layer["W"].shape
        small = n <= self.local_batch_cols or (n <= 2 * self.local_batch_cols and R <= 1024)
        return self.local_batch > 1 and small and self._plain_order()

    def wants_stacked_loop(self, layer):
        """Wide layers with few rows (OPT-350M / BLOOM-560M's 1024 x 4096): the n^3 factorisation fills the chip, the loop
        does not -- its window kernel runs one workgroup per 16 rows, 64 of them for 1024 rows.  Such layers are
        factored one by one on the factor streams and LOOPED in stacks of 4096 rows (run_round_stacked)."""
        R, n = layer["W"].shape
        return self.local_batch > 1 and not self.wants_local_batch(layer) and R <= 2048 and self._plain_order()

    def run_round_stacked(self, round_layers, factors):
        """All rows of a round's layers from their own factors (order, U, info[, symmetry flag]) made elsewhere on this
        GPU: stacked, then ONE loop / error over all of them."""
        order, U = [f[0] for f in factors], [f[1] for f in factors]  # (stacked by _run_stacked only where a stack is needed)
        info = torch.cat([f[2] for f in factors])
        known = torch.cat([f[3] for f in factors]) if all(len(f) > 3 for f in factors) else None
        return self._run_stacked(round_layers, 0, round_layers[0]["W"].shape[0], order, U, info, known)

    def run_round_local(self, round_layers):
        """All rows of a round's layers on this rank: batched factorisation (engine.factorize_batch), then the
        stacked loop / local search / error of run_round."""
        eng = self.engine
        n = round_layers[0]["H"].shape[0]
        order, U, info = eng.factorize_batch([lay["H"] for lay in round_layers], n, self.damp, eng.order_mode_code(self.act_order))
        return self._run_stacked(round_layers, 0, round_layers[0]["W"].shape[0], order, U, info, None)

    def _run_stacked(self, round_layers, lo, hi, order, U, info, known):
        """Rows [lo, hi) of every layer of the round through ONE loop and ONE error evaluation, from the layers' factors --
        stacked, order (B, n), U (B, n, n), or a list of each, one per layer -- and info (B,); known: the symmetry verdicts of
        the Hessians, or None (checked here)."""
        eng = self.engine
        B, n = len(round_layers), round_layers[0]["H"].shape[0]
        device = round_layers[0]["W"].device
        rows = hi - lo
        Rp = (rows + 127) // 128 * 128  # the batch entry points want whole 128-row tiles per layer (96 rows at 768 / 8)
        Hs = [lay["H"] for lay in round_layers]
        carried = self._carried_error(round_layers)
        # Whole tiles, row scales or none, no search and no product of the error: the loop is all there is, and it reads every
        # layer's W, scale, order and U where they lie (engine.gptq_loop with lists) -- no copy into stacks (six 4096-column
        # factors that were not made by one batched factorisation: 0.8 GB read and written).
        if (rows == Rp and B <= LOOP_LAYERS and round_layers[0].get("gscale") is None and self.moves == 0
                and (carried == "loop" or not self.with_error)):
            return self._shards(round_layers, lo, hi, self._loop_layers(round_layers, lo, hi, list(order), list(U), carried == "loop"), info.split(1))
        if isinstance(order, list):
            order, U = _stack_views(order), _stack_views(U)  # (factors that came out of ONE batched factorisation are a stack already)
        # ragged shard: every layer's rows padded to whole tiles (zero weights, unit scales); rows never interact, so the
        # padding rows are wasted work and nothing else -- they are cut off below.  One launch per stack either way
        # (engine.stack_rows: a copy per layer was 120 small launches per step for one rank of 8 on OPT-125M).

        def stacked(key, fill):
            if round_layers[0].get(key) is None:
                return None
            return eng.stack_rows([lay[key][lo:hi] for lay in round_layers], Rp, fill)

        W, sc, S = stacked("W", 0.0), stacked("scale", 1.0), stacked("gscale", 1.0)
        cb = eng.require_uniform(self.quantizer)
        want_idx = cb[0] <= 256  # (the kernels emit uint8 indices)
        if self.moves > 0 and S is None:
            # local search works in the scaled domain (engine.quantize_layer): scaled copy in, ONE search over the stack
            # (engine.local_search_batch: a search per layer is ten small launches, and the shards of a round on several
            # ranks are a few hundred rows each), de-scale on the way out.  (Padding rows of a ragged shard search too:
            # rows never interact, they are cut off below.)
            Ws = eng.rows_divide(W.view(B * Rp, n), sc.reshape(-1)).view(B, Rp, n) if sc is not None else W
            Q, idx, _, _ = eng.gptq_loop(Ws, cb, order, U, *self.blocks, want_idx=want_idx)
            # vouched Hessians: the search carries every row's error with it (obq.py:254, 290 -- the gain of a move IS the
            # change of the error when H is symmetric), so the layer error needs no product of its own; it comes out in the
            # scaled domain, (W - Qw) = scale (Ws - Q): times scale^2.
            # Per row it is as exact as the reference's own `ls.err` (float32 gains: a few 1e-5 relative on a rare row), the
            # layer's mean agrees with the recomputed product to ~1e-8 (BLOOM-560M, all 96 layers).
            err = torch.empty((B, Rp), dtype=torch.float32, device=device) if carried == "search" else None
            eng.local_search_batch(Ws, Q, Hs, cb, self.moves, idx if want_idx else None, known, err)
            if sc is not None:
                Q = eng.rows_divide(Q.view(B * Rp, n), sc.reshape(-1), invert=True).view(B, Rp, n)
                if err is not None:
                    err = (err * sc) * sc
        else:
            # the loop de-scales itself here whatever the order (group scales: it runs on the unscaled weights and Q comes back
            # de-scaled), so a carried error is that of the Q returned, and so is the product's
            Q, idx, _, err = eng.gptq_loop(W, cb, order, U, *self.blocks, scale=sc, gscale=S, group_size=round_layers[0].get("group_size"),
                                           want_idx=want_idx, unscale=sc is not None, Hs=Hs if carried == "loop" else None, damp=self.damp)
        if self.with_error and err is None:
            err = eng.row_errors_batch(W, Q, Hs, known)
        return self._shards(round_layers, lo, hi, (Q, idx if want_idx else None, err), info.split(1))

    @staticmethod
    def _shards(round_layers, lo, hi, stacks, infos):
        """A loop's stacked results (Q, idx, row_err: (B, padded rows, ...), idx / row_err may be None) as one shard per layer,
        each with its layer's factorisation status word."""
        Q, idx, err = stacks
        rows = hi - lo
        return [dict(Q=Q[b, :rows], idx=None if idx is None else idx[b, :rows], row_err=None if err is None else err[b, :rows],
                     rows=(lo, hi), info=infos[b]) for b in range(len(round_layers))]

    def _loop_layers(self, stack_layers, lo, hi, orders, Us, carry, latency=False):
        """Rows [lo, hi) of same-shaped layers (row scales or none) through ONE loop that reads every layer's tensors where they
        lie; carry: the loop carries the rows' errors (_carried_error "loop").  Returns the stacked (Q, idx, row_err)."""
        eng = self.engine
        cb = eng.require_uniform(self.quantizer)
        scaled = stack_layers[0].get("scale") is not None
        Q, idx, _, err = eng.gptq_loop([lay["W"][lo:hi].contiguous() for lay in stack_layers], cb, orders, Us, *self.blocks,
                                       scale=[lay["scale"][lo:hi].contiguous() for lay in stack_layers] if scaled else None,
                                       want_idx=cb[0] <= 256, unscale=scaled, latency=latency,
                                       Hs=[lay["H"] for lay in stack_layers] if carry else None, damp=self.damp)
        return Q, idx, err

    # -- one rank, full-height layers: `tall_stack` consecutive ones of a shape and kind share ONE set of loop launches
    # A window launch of one 4096-row layer is 128 workgroups of 32 rows, each alone on its CU (158 KB of LDS): half the chip,
    # left to the factor streams' kernels to fill -- which the streams that share the loop stream's hardware queue cannot (at 4
    # queues a third of the factorisations).  Two layers are 256 workgroups, the whole chip for the same duration; four are two
    # full rounds and a quarter of the launches.  The loop reads every layer where it lies (_loop_layers): nothing is copied.
    # Headline, ms per step, alternating with the parent: 24.15 layer by layer, 21.49 in stacks of 2, 21.20 of 4 (DESIGN.md 8.9;
    # with `--streams 2,1`, where nothing shares the loop stream's queue, the stacks lose 0.9 ms instead).  1: layer by layer
    # (run_rows).
    tall_stack = 4

    def wants_tall_stack(self, layer):
        """Layers whose loop may share its launches with the next ones of the same shape and kind (quantize_stream's
        layer-by-layer route on one rank): plain orders, row scales or none, no search, the error carried by the loop."""
        return (self.tall_stack > 1 and self._plain_order() and self.moves == 0 and layer.get("gscale") is None
                and layer["W"].shape[0] % 64 == 0 and self._carried_error([layer]) == "loop")

    def run_tall(self, stack_layers, factors):
        """All rows of up to tall_stack same-shaped layers from their own factors through one loop: the shards of run_rows."""
        R = stack_layers[0]["W"].shape[0]
        stacks = self._loop_layers(stack_layers, 0, R, [f[0] for f in factors], [f[1] for f in factors], True, latency=not self.overlap)
        return self._shards(stack_layers, 0, R, stacks, [f[2] for f in factors])


LOOP_LAYERS = 16  # layers one loop takes as a list of tensors (slk_gptq_quantize_layers)


class _Lanes:
    """The streams of ONE quantize_stream call and every operation the scheduler makes on them: the only code of the module
    that touches torch.cuda's streams and events or Tensor.record_stream (but for _all_gather_words and its rehearsal handle).
    With no side streams (overlap=False, the CPU stand-ins) every stream it hands out is None and every verb does nothing."""

    def __init__(self, backend=None, join=True):
        self.backend, self.joins = backend, join
        fs, self.comm, ls = backend.streams() if backend is not None else (None, None, None)
        self.factor, self.loop, self.side = fs or [], ls or [], fs is not None
        self.here = torch.cuda.current_stream() if self.side else None
        self.pool = (self.factor + self.loop) or [None]  # what the one-rank rounds of small layers alternate over
        self._forked = set()

    def _take(self, counter, streams):
        if not self.side:
            return None
        k = getattr(self.backend, counter)  # the rotation lives on the backend: it carries on from one call to the next
        setattr(self.backend, counter, (k + 1) % len(streams))
        return streams[k % len(streams)]

    def next_factor(self):
        """Factorisations are latency-bound chains: consecutive ones alternate between the factor streams (across calls too:
        with one layer per rank and call, consecutive calls would otherwise queue one chain behind the other)."""
        return self._take("_factor_rotation", self.factor)

    def next_loop(self):  # batched rounds rotate over the loop streams across calls, like the factorisations
        return self._take("_loop_rotation", self.loop)

    def loop_of(self, l):  # layer by layer: consecutive layers alternate
        return self.loop[l % len(self.loop)] if self.side else None

    def fork(self, *streams):
        """Each of `streams` behind the caller's stream, once per call (before its first use)."""
        for st in streams:
            if st is not None and id(st) not in self._forked:
                self._forked.add(id(st))
                st.wait_stream(self.here)

    def on(self, stream, layers=()):
        """Context: what is enqueued inside goes to `stream` and reads the caller's tensors of `layers`.  Unjoined, the caching
        allocator is told so: a caller who drops them right after a join=False call does not hand memory the side streams
        still read back for reuse (the allocator holds the block until `stream` has passed this point)."""
        if stream is None:
            return contextlib.nullcontext()
        if not self.joins:
            for lay in layers:
                for key in ("W", "H", "scale", "gscale", "mean"):
                    t = lay.get(key)
                    if isinstance(t, torch.Tensor) and t.is_cuda:
                        t.record_stream(stream)
        return torch.cuda.stream(stream)

    def mark(self, stream):
        """An event at this point of `stream` (None: none)."""
        if stream is None:
            return None
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    @staticmethod
    def stamp():
        """Measurement (exchange_log): a timing event at this point of the current stream, side streams or not."""
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def wait(self, stream, event):
        if event is not None:
            stream.wait_event(event)

    def moved(self, tensors, stream):
        """`tensors` were made on one stream and are read on `stream` (lanes.here: the caller's): keep the allocator honest."""
        if stream is not None:
            for t in tensors:
                if isinstance(t, torch.Tensor):
                    t.record_stream(stream)

    def join(self, streams):
        """join=True: the caller's stream waits for `streams`, so the results can be used on it at once."""
        if self.joins and self.here is not None:
            for st in streams:
                self.here.wait_stream(st)


def _stack_views(tensors):
    """torch.stack -- or, when the tensors already lie one behind the other in one allocation (slices of a batched result),
    a view of that allocation: no copy (six 4096-column factors are 0.8 GB)."""
    t0 = tensors[0]
    step = t0.numel()
    base = t0.untyped_storage().data_ptr()
    if t0.is_contiguous() and all(t.is_contiguous() and t.shape == t0.shape and t.dtype == t0.dtype and t.untyped_storage().data_ptr() == base
                                  and t.storage_offset() == t0.storage_offset() + i * step for i, t in enumerate(tensors)):
        return t0.as_strided((len(tensors),) + tuple(t0.shape), (step,) + tuple(t0.stride()))
    return torch.stack(tensors)


def _all_gather_words(payload, size):
    """All-gather equal-sized int64 buffers; returns (list of per-rank views, async work)."""
    if rehearse is not None:
        ev = None
        if payload.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
        return [payload] * size, _Done(ev)
    if dist.get_backend() == "nccl":
        out = torch.empty(size * payload.numel(), dtype=payload.dtype, device=payload.device)
        work = dist.all_gather_into_tensor(out, payload, async_op=True)
        return list(out.chunk(size)), work
    outs = [torch.empty_like(payload) for _ in range(size)]
    return outs, dist.all_gather(outs, payload, async_op=True)


def _shape_kind(layer):
    """The key of short rounds, groups of rounds and tall stacks: layers of one key may share a loop."""
    return tuple(layer["W"].shape), _layer_kind(layer)


def _chain_cap(backend, n):
    """How many n-column factorisations may share one launch chain (factorize_many): a chain of B holds B x (A, U and two
    workspace images) of n x n doubles, capped at backend.group_bytes."""
    return max(1, int(backend.group_bytes) // (32 * n * n))


def _factor_job(lanes, backend, job):
    """The factors of a job's layers on the next factor stream -- one launch chain for several (factorize_many), the plain
    call for one -- with the event behind them and the stream they went to."""
    fs = lanes.next_factor()
    lanes.fork(fs)
    with lanes.on(fs, job):
        made = backend.factorize_many(job) if len(job) > 1 else [backend.factorize(job[0])]
        return made, lanes.mark(fs), fs


def _run_layer(backend, layer, factor, rank=0, size=1):
    """A single layer's rows of `rank` from its factor: the shard, with the factorisation's status word."""
    return dict(backend.run_rows(layer, *row_range(layer["W"].shape[0], rank, size), factor), info=factor[2])


def _quantize_stream_local(layers, small, short, backend, join):
    """One rank, a stream with small or short layers in it (quantize_stream).  `small` layers go in batched rounds by
    shape -- factored AND looped together -- one round after the other on alternating streams (a round is a chain of short
    launches: two or three in flight fill the gaps); `short` ones (wide, few rows) go in rounds whose factorisations share
    one launch chain on a factor stream (HipBackend.short_factor_batch) and whose rows are looped as one stack; the rest
    through the usual route."""
    out = [None] * len(layers)
    lanes = _Lanes(backend, join)
    lanes.fork(*lanes.pool)

    def keep(shards, idxs):
        for l, shard in zip(idxs, shards):
            out[l] = shard
        lanes.moved([t for shard in shards for t in shard.values()], lanes.here)  # made on a side stream, consumed on the caller's

    for i, members in enumerate(plan_rounds([layers[l] for l in small], backend.local_batch)[0] if small else []):
        st = lanes.pool[i % len(lanes.pool)]
        idxs = [small[m] for m in members]
        round_layers = [layers[l] for l in idxs]
        with lanes.on(st, round_layers):
            if len(idxs) == 1:
                shards = [_run_layer(backend, round_layers[0], backend.factorize(round_layers[0]))]
            else:
                shards = backend.run_round_local(round_layers)
        keep(shards, idxs)
    # a short round's factorisations in launch chains (the chains rotate over the factor streams), its stacked loop on the
    # loop stream behind them
    ls = lanes.loop_of(0)
    for members in _short_rounds(layers, short, backend):
        round_layers = [layers[l] for l in members]
        per_chain = max(1, min(int(backend.short_factor_batch), _chain_cap(backend, round_layers[0]["H"].shape[0])))
        facs, events = [], []
        for i in range(0, len(members), per_chain):
            made, ev, _ = _factor_job(lanes, backend, round_layers[i:i + per_chain])
            facs.extend(made)
            events.append(ev)
        with lanes.on(ls, round_layers):
            for ev in events:
                lanes.wait(ls, ev)
            if len(members) == 1:
                shards = [_run_layer(backend, round_layers[0], facs[0])]
            else:
                shards = backend.run_round_stacked(round_layers, facs)
            for f in facs:
                lanes.moved(f, ls)
        keep(shards, members)
    taken = set(small) | set(short)
    rest = [l for l in range(len(layers)) if l not in taken]
    if rest:
        for l, shard in zip(rest, _quantize_stream([layers[l] for l in rest], backend, join=join, _local=False)):
            out[l] = shard
    lanes.join(lanes.pool)
    return out


def _short_rounds(layers, short, backend):
    """Rounds of same-shaped `short` layers whose stacked rows come to about a full layer's worth (4096)."""
    by_shape = {}
    for l in short:
        by_shape.setdefault(_shape_kind(layers[l]), []).append(l)
    rounds = []
    for (shape, _), members in by_shape.items():
        per = max(2, min(backend.local_batch, int(backend.short_rows) // max(shape[0], 1)))
        rounds.extend(members[i:i + per] for i in range(0, len(members), per))
    return rounds


def quantize_stream(layers, backend, comm_device=None, join=True):
    """Quantize `layers` (see _quantize_stream) and REGISTER every layer's factorisation status.

    A Hessian that is not positive definite makes the reference raise numpy.linalg.LinAlgError
    (sleekit/obq.py:49-50, np.linalg.cholesky).  Here the status word of every layer's factorisation --
    made on this rank, or carried by the packed factor another rank sent -- is handed to the backend
    (`backend.note_status`): HipBackend raises LinAlgError naming the layer, at once when `join` is true and
    sleekit_amd._device.lazy_errors is off (the default), otherwise at `_device.raise_pending()`.  Every rank sees
    every layer's status, so every rank raises.

    join=True ends in ONE blocking device -> host read of the status words (a host synchronisation per call).  join=False
    blocks nowhere: `_device.raise_pending()` is then REQUIRED, after synchronising, to see the statuses (the list it reads is
    bounded: _device.PENDING_LIMIT); the inputs may be dropped at once (_Lanes.on).

    Group scales: a layer dict may carry `gscale` (R, n / group_size) float32 and `group_size` instead of `scale`; its shards
    are then those of sleekit_amd.groups (Q de-scaled, idx the codebook indices of Q / s).  check_layers refuses bad keys
    (ValueError) and grouped layers under a local search (NotImplementedError) before anything runs.
    """
    check_layers(layers, backend.moves)
    out = _quantize_stream(layers, backend, comm_device, join, True)
    backend.note_statuses([None if shard is None else shard.get("info") for shard in out], layers, defer=not join)
    return out


def _group_rounds(rounds, layers, backend, rank, size):
    """Consecutive rounds of one shape joined into groups of at most backend.group_limit(layer, shard rows) layers (the
    loop batch the backend wants for such shards); for a backend that wants none (Backend.group_limit: 0), or for big layers
    (limit below two rounds), every round is a group of its own."""
    groups, key_now, count, limit = [], None, 0, 0
    for g, members in enumerate(rounds):
        first = layers[members[0]]
        key = _shape_kind(first) if len({_shape_kind(layers[l]) for l in members}) == 1 else None
        if key is not None and key == key_now and count + len(members) <= limit:
            groups[-1].append(g)
            count += len(members)
            continue
        groups.append([g])
        key_now, count = key, len(members)
        # The limit must be the SAME on every rank: it decides how many all-gathers there are and how large.  Shard heights
        # differ by one when R % size != 0 (1030 rows on 8 ranks: 129 / 128, on either side of the 128-row padding), so every
        # rank asks with the TALLEST shard, rank 0's = ceil(R / size) -- also for a rank that has no rows of the layer at all.
        lo, hi = row_range(first["W"].shape[0], 0, size)
        limit = int(backend.group_limit(first, hi - lo)) if key is not None else 0
    return groups


def _factor_jobs(groups, rounds, root, rank, layers, backend):
    """The factorisations `rank` owes -- the layers it is the root of, in processing order -- as lists of layers factored
    together: its layers of a GROUP of rounds share one launch chain (up to _chain_cap of them) when the backend factors in
    chains, everything else goes one by one."""
    jobs = []
    for members_g in groups:
        own = [l for g in members_g for l in rounds[g] if root[l] == rank]
        if len(members_g) > 1 and len(own) > 1 and backend.factor_chains:
            cap = _chain_cap(backend, layers[own[0]]["H"].shape[0])
            jobs.extend(own[i:i + cap] for i in range(0, len(own), cap))
        else:
            jobs.extend([l] for l in own)
    return jobs


def _tall_stacks(order, layers, backend):
    """One rank: consecutive full-height layers of one shape and kind share one loop (backend.tall_stack at a time; a
    remainder goes through the same call with fewer).  Returns tall[first member] = the stack, tall[later member] = ()."""
    tall = {}
    per = min(int(backend.tall_stack), LOOP_LAYERS)
    run, run_key = [], None
    for l in list(order) + [None]:
        key = None if l is None or not backend.wants_tall_stack(layers[l]) else _shape_kind(layers[l])
        if key != run_key or len(run) == per:
            for m in run:
                tall[m] = run if m == run[0] else ()
            run = []
        run_key = key
        if key is not None:
            run.append(l)
    return tall


_Plan = collections.namedtuple("_Plan", "rank size exchange rounds root groups slot jobs tall")


def _plan_stream(layers, backend, rank, size):
    """Who does what, from the layers, the world and the backend's policy alone (no stream, no tensor is touched).

    rounds of one shape each and root[l] = the rank that factors layer l (plan_rounds).  Rounds of SMALL layers are taken in
    GROUPS (the backend says how many layers it wants in one loop batch: group_limit): a rank factors all its layers of a
    group in one batched factorisation (jobs), the group's payloads cross in ONE all-gather (slot[l]: the slot of l's round in
    every rank's buffer) and its row shards go through the loop as ONE stack.  The shards of a small layer on several ranks
    are a chain of short launches whatever their height (one rank of 8 on OPT-125M: 10 rounds x 15 loop launches and 9
    factorisations x 45 launches per step, as long as the whole model on one GPU); groups make it 3 x 15 and 3 x 45.  A group
    of one round is the plain scheme."""
    exchange = size > 1 or always_exchange
    rounds, root = plan_rounds(layers, size, bucket=exchange and backend.bucket_by_shape)
    groups = _group_rounds(rounds, layers, backend, rank, size) if exchange else [[g] for g in range(len(rounds))]
    slot = {l: j for members_g in groups for j, g in enumerate(members_g) for l in rounds[g]}
    jobs = _factor_jobs(groups, rounds, root, rank, layers, backend)
    tall = {} if exchange else _tall_stacks([l for g in rounds for l in g], layers, backend)
    return _Plan(rank, size, exchange, rounds, root, groups, slot, jobs, tall)


def _factor_phase(run):
    """1. every rank factors the layers it is the root of (concurrently across ranks), job by job on rotating factor
    streams; factors[l], the event behind it (ready[l]) and the stream it went to (stream_of[l])."""
    for job in run.plan.jobs:
        made, ev, fs = _factor_job(run.lanes, run.backend, [run.layers[l] for l in job])
        for l, fac in zip(job, made):
            run.factors[l], run.ready[l], run.stream_of[l] = fac, ev, fs


def _exchange_group(layers, group_rounds, root, rank, size, backend, lanes, factors, ready, device):
    """The all-gather of one group of rounds (lists of layers), asynchronous: this rank's payload of every round -- its own
    layer's packed factor, behind that factor's event -- in the round's slot of one buffer of equal-sized contributions.
    Returns (buffer, (per-rank buffers, work, words per payload, words per slot))."""
    # equal-sized contributions: a group's layers share one shape (a lone round of mixed shapes: the widest)
    words = max(backend.payload_words(layers[l]["H"].shape[0]) for members in group_rounds for l in members)
    stride = (words + 1) // 2 * 2 if len(group_rounds) > 1 else words
    buffer = None if len(group_rounds) == 1 else backend.alloc_payload(stride * len(group_rounds), device)
    for j, members in enumerate(group_rounds):
        own = [l for l in members if root[l] == rank]  # at most one: a round has at most `size` layers
        if own:
            l = own[0]
            lanes.wait(lanes.comm, ready[l])
            payload = backend.pack(factors[l], words)
            lanes.moved(factors[l], lanes.comm)  # made on a factor stream, read here
        elif rehearse is not None:
            # rehearsal: a real factor of the right shape must stand in for the peers' (a blank one is not a
            # permutation + triangle the kernels can run on); made once per shape, outside what is measured
            first = layers[members[0]]
            key = (first["H"].shape[0], words)
            if key not in _rehearsal_payloads:
                _rehearsal_payloads[key] = backend.pack(backend.factorize(first), words)
            payload = _rehearsal_payloads[key]
        elif buffer is None:  # no layer of this round is this rank's: contribute a blank
            payload = backend.alloc_payload(words, device).zero_()
        else:
            payload = None  # (a slot nobody reads)
        if buffer is None:
            buffer = payload
        elif payload is not None:
            buffer[j * stride:j * stride + words].copy_(payload)
    log = backend.exchange_log
    if log is not None and buffer.is_cuda:
        # measurement (bench.py's pass with events): the comm stream brackets the collective with two events
        # and waits for it, so that their distance is the exchange itself
        e0 = lanes.stamp()
        parts, work = _all_gather_words(buffer, size)
        work.wait()
        log.append((e0, lanes.stamp(), buffer.numel() * buffer.element_size() * (size - 1)))
    else:
        parts, work = _all_gather_words(buffer, size)
    return buffer, (parts, work, words, stride)


def _exchange_phase(run, comm_device):
    """2. one asynchronous all-gather per group of rounds, issued in order on the comm stream."""
    plan, lanes = run.plan, run.lanes
    lanes.fork(lanes.comm)
    with lanes.on(lanes.comm):
        for gi, members_g in enumerate(plan.groups):
            device = comm_device if comm_device is not None else run.layers[0]["H"].device
            buffer, run.gathered[gi] = _exchange_group(run.layers, [plan.rounds[g] for g in members_g], plan.root, plan.rank, plan.size,
                                                       run.backend, lanes, run.factors, run.ready, device)
            run.buffers.append(buffer)


def _payload_of(run, gi, l):
    parts, _, words, stride = run.gathered[gi]
    at = run.plan.slot[l] * stride
    return parts[run.plan.root[l]][at:at + words]


def _loop_phase(run):
    """3. every rank runs its rows of every layer as the factors land, group by group.  A group goes through the
    kernels as ONE batch when the backend can do that (run_round): the shards are R / G rows each, too few to
    fill the chip alone.  Otherwise layer by layer, consecutive ones on alternating streams (their leaf chains
    are latency-bound) -- on one rank in stacks where the backend wants them (run_tall)."""
    plan = run.plan
    run.lanes.fork(*run.lanes.loop)
    for gi, members_g in enumerate(plan.groups):
        members = [l for g in members_g for l in plan.rounds[g]]
        round_layers = [run.layers[l] for l in members]
        lo, hi = row_range(round_layers[0]["W"].shape[0], plan.rank, plan.size)
        if plan.exchange and run.backend.can_batch(round_layers, lo, hi):
            _loop_round(run, gi, members, round_layers, lo, hi)
            continue
        for l in members:
            if l not in plan.tall:
                _loop_layer(run, gi, l)
            elif plan.tall[l]:  # (a later member went with the first)
                _loop_tall(run, plan.tall[l])


def _loop_round(run, gi, members, round_layers, lo, hi):
    """A group's shards as one batch, from the payloads of its all-gather."""
    lanes = run.lanes
    ls = lanes.next_loop()
    own = [l for l in members if l in run.stream_of]
    if own and run.backend.rounds_on_factor_streams:
        # The round runs on the stream that factored this rank's layer of it: one stream fewer to pair badly.
        # HIP multiplexes all streams of a process onto a few in-order hardware queues; a loop stream that shares
        # its queue with the factor stream of the NEXT round puts that factorisation behind this round's loops and
        # the pipeline collapses into factor -> loop -> factor (4.4 ... 7.0 ms per step at N = 8 depending on how
        # the streams fell).
        ls = run.stream_of[own[0]]
    with lanes.on(ls, round_layers):
        parts, work = run.gathered[gi][:2]
        work.wait()  # orders the stream behind the transfer; no host block on GPU
        shards = run.backend.run_round(round_layers, lo, hi, [_payload_of(run, gi, l) for l in members])
        lanes.moved(parts, ls)
    for l, shard in zip(members, shards):
        run.out[l] = shard


def _loop_tall(run, stack):
    """One rank: a stack of full-height layers through one loop, behind EVERY member's factorisation."""
    lanes = run.lanes
    ls = lanes.loop_of(stack[0])
    stack_layers = [run.layers[m] for m in stack]
    with lanes.on(ls, stack_layers):
        for m in stack:
            lanes.wait(ls, run.ready[m])
        for m, shard in zip(stack, run.backend.run_tall(stack_layers, [run.factors[m] for m in stack])):
            run.out[m] = shard
        for m in stack:
            lanes.moved(run.factors[m], ls)  # made on the factor streams, read on this one


def _loop_layer(run, gi, l):
    """A single layer's rows: from its factor made here, or from the payload of its round's all-gather."""
    plan, lanes, layer = run.plan, run.lanes, run.layers[l]
    ls = lanes.loop_of(l)
    with lanes.on(ls, [layer]):
        if plan.exchange:
            parts, work = run.gathered[gi][:2]
            work.wait()
            if run.factors[l] is None or always_exchange:
                run.factors[l] = run.backend.unpack(_payload_of(run, gi, l), layer["H"].shape[0])
        else:
            lanes.wait(ls, run.ready[l])
        run.out[l] = _run_layer(run.backend, layer, run.factors[l], plan.rank, plan.size)
        lanes.moved(run.factors[l], ls)  # made on a factor / comm stream, read on this one
        if plan.exchange:
            lanes.moved(parts, ls)


def _quantize_stream(layers, backend, comm_device=None, join=True, _local=True):
    """Quantize `layers` (list of dicts with W (R, n), H (n, n), optional scale (R,) or gscale / group_size) across the ranks.

    Returns, per layer, this rank's shard: dict(Q, idx, row_err, rows=(lo, hi), info).
    Every rank holds every layer's inputs (W, H are inputs of the path and resident before
    it starts); only the factor travels.

    Layers are taken in ROUNDS of at most G (= world size) layers of ONE shape (plan_rounds: the stream is
    bucketed by shape first, since a model's layer order mixes shapes and the layers are independent); the
    ranks factor one layer of the round each, then ONE collective per round exchanges the packed factors
    (status, order, upper triangle of U: n (n + 1) / 2 + n + 1 words per layer).  It is an all-gather -- G simultaneous one-to-all
    broadcasts -- because xGMI is a point-to-point mesh: every rank then receives over all of its
    7 links at once, where G separate ring broadcasts would each crawl through one link per hop.

    Three kinds of queues per rank when the backend provides device streams (`backend.streams()`, held by _Lanes):
      factor streams : the n x n factorisations this rank owns (latency-bound chains)            _factor_phase
      comm stream    : pack + all-gather of each round, behind that round's factor event         _exchange_phase
      loop streams   : the row loops, each behind its round's collective                         _loop_phase
    so the factorisation of round g+1 runs under the loops and errors of round g.

    `join` (default): the caller's stream waits for the loop streams before this returns, so the results can
    be used on it at once.  With join=False nothing waits: the NEXT call's factorisations then start under
    this call's loops (a throughput loop over independent batches, bench.py) -- synchronise the device, or
    the loop streams, before reading the results.  The INPUT tensors may be dropped when the call returns: every side
    stream that reads them is recorded on them (_Lanes.on), so their memory is not reused before those streams pass.
    """
    rank, size = world()
    n_layers = len(layers)
    if size == 1 and not always_exchange and _local:
        # one rank: small layers go in rounds of one shape, factored and looped in launches that cover the round
        small = [l for l in range(n_layers) if backend.wants_local_batch(layers[l])]
        short = [l for l in range(n_layers) if backend.wants_stacked_loop(layers[l])]
        small, short = (small if len(small) > 1 else []), (short if len(short) > 1 else [])
        if small or short:
            return _quantize_stream_local(layers, small, short, backend, join)
    plan = _plan_stream(layers, backend, rank, size)
    lanes = _Lanes(backend, join)
    run = types.SimpleNamespace(layers=layers, backend=backend, plan=plan, lanes=lanes, factors=[None] * n_layers, ready=[None] * n_layers,
                                stream_of={}, gathered=[None] * len(plan.groups), buffers=[], out=[None] * n_layers)
    _factor_phase(run)
    if plan.exchange:
        _exchange_phase(run, comm_device)
    _loop_phase(run)
    lanes.join(lanes.loop + lanes.factor)  # (batched rounds run on factor streams)
    # tensors made on the side streams are consumed on the caller's stream
    lanes.moved([t for f in run.factors if f is not None for t in f] + [b for b in run.buffers if b is not None]
                + [t for got in run.gathered if got is not None for t in got[0]] + [t for shard in run.out for t in shard.values()], lanes.here)
    return run.out


def verify_exchange(layers, backend, max_rounds=2):
    """Self-check of the collective: for the first rounds of the stream, every rank packs the factor of its own layer,
    the payloads are all-gathered exactly as quantize_stream does, and every rank's copy of every payload is held to its
    ROOT's own buffer by two wrapping int64 checksums (plain and position-weighted), compared across ranks through a
    second, tiny all-gather.  Returns dict(world_size, backend, rounds_checked, payload_bytes, agree)."""
    rank, size = world()
    out = dict(world_size=size, backend=dist.get_backend() if size > 1 and rehearse is None else "none", rounds_checked=0,
               payload_bytes=0, agree=True)
    if size <= 1 or rehearse is not None:
        return out
    rounds, root = plan_rounds(layers, size)
    for members in rounds[:max_rounds]:
        # this rank's payload of the round and its all-gather, by the scheduler's own function (on the current stream)
        factors = {l: backend.factorize(layers[l]) for l in members if root[l] == rank}
        payload, (parts, work, words, _) = _exchange_group(layers, [members], root, rank, size, backend, _Lanes(), factors,
                                                           dict.fromkeys(factors), layers[0]["H"].device)
        work.wait()
        weight = torch.arange(1, words + 1, dtype=torch.int64, device=payload.device)

        def sums(t):
            return torch.stack([t.sum(), (t * weight).sum()])

        seen = torch.stack([sums(p) for p in parts])  # (size, 2): this rank's view of every rank's payload
        views = [torch.empty_like(seen) for _ in range(size)]
        dist.all_gather(views, seen)
        views = torch.stack(views).cpu()  # [viewer][source][2]
        mine = sums(payload).cpu()
        ok = bool(torch.equal(views[rank][rank], mine))
        for src in range(size):
            ok = ok and all(bool(torch.equal(views[viewer][src], views[src][src])) for viewer in range(size))
        out["agree"] = out["agree"] and ok
        out["rounds_checked"] += 1
        out["payload_bytes"] = int(words * 8)
    return out


def layer_error(shards_row_err, R):
    """Mean over all R rows of a layer from this rank's row errors (sum-all-reduce of one scalar).

    Bookkeeping outside the timed path: the reference's layer error is the host-side mean.
    """
    total = shards_row_err.double().sum()
    rank, size = world()
    if size > 1:
        dist.all_reduce(total)
    return total / R
