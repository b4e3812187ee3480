#!/usr/bin/env python3
"""What sleekit_amd.dist.quantize_stream ENQUEUES, one line per operation: run it on two checkouts and diff the files to hold a
change of the scheduler to "same backend calls, same arguments, same order, same streams, same events, same record_stream".

    python tools/stream_trace.py [--tree PATH] [--out DIR] [--cpu]

Only torch is patched (torch.cuda.stream, Stream.wait_stream / wait_event, Event.record, Tensor.record_stream, the all-gathers
of torch.distributed) and the backend's entry points are wrapped ON THE INSTANCE, so the same file runs against either tree:
`--tree PATH` puts that tree's sleekit_amd (and, with --cpu, its tests' stand-in backends) first.  Names are normalised --
streams as caller / f0.. / c / l0.., events by order of first use, tensors by dtype and shape (a factor's by the layer it is
of), layers by index -- and every scenario runs TWO consecutive calls per stream of layers, so that the rotation carried from
one call to the next shows.  One text file per scenario under DIR (default stream_traces/).

Default (GPU box, HipBackend): one rank with small / short-wide / plain layers, joined and not, on (3, 1), (2, 2) and no side
streams; tall stacks of 1, 2, 4; one rank of 2, 4, 8 rehearsed with the rounds on the factor streams and off them (model-order
stream, a group of four rounds, wide layers in a group, 1030 ragged rows), with an exchange log and with local-search moves;
always_exchange under a one-rank gloo group.  Fails if one of the nine entry points shows in no trace.
--cpu (no GPU): the stand-in backends of tests/test_dist_gloo.py on one rank, rehearsed, and on a 2-rank gloo world.
"""
import argparse
import contextlib
import importlib.util
import os
import socket
import sys

import torch

ENTRY = ("factorize", "factorize_many", "pack", "unpack", "run_rows", "run_round", "run_round_local", "run_round_stacked", "run_tall")
ALSO = ("alloc_payload",)


class Trace:
    """The lines of one scenario and the names given so far."""

    def __init__(self, layers=(), streams=None):
        self.lines, self.events, self.tags, self.held, self.serial = [], {}, {}, [], {}
        self.layers = {id(lay): f"L{i}" for i, lay in enumerate(layers)}
        self.streams = streams or {}

    def log(self, text):
        self.lines.append(text)

    def stream(self, st):
        if st is None:
            return "None"
        return self.streams.setdefault(st.cuda_stream, f"s{len(self.streams)}")

    def here(self):
        return f" @{self.stream(torch.cuda.current_stream())}" if self.streams else ""

    def event(self, ev):
        if id(ev) not in self.events:
            self.events[id(ev)] = f"e{len(self.events)}"
            self.held.append(ev)  # (an id is a name only while the object lives)
        return self.events[id(ev)]

    def tag(self, value, kind):
        """Name the tensors of a backend's result (a factor: F<layer>.<j>; an unpacked one: U<k>.<j>; a payload: P<k>)."""
        if kind in self.layers.values():
            kind = "F" + kind[1:]
        else:
            k = self.serial[kind] = self.serial.get(kind, -1) + 1
            kind = f"{kind}{k}"
        for j, t in enumerate(value if isinstance(value, (tuple, list)) else (value,)):
            if isinstance(t, torch.Tensor):
                self.tags[id(t)] = f"{kind}.{j}"
                self.held.append(t)

    def show(self, x):
        if isinstance(x, torch.Tensor):
            if id(x) in self.tags:
                return self.tags[id(x)]
            off = f"@{x.storage_offset()}" if x.storage_offset() else ""
            return f"{str(x.dtype).replace('torch.', '')}{list(x.shape)}{off}".replace(" ", "")
        if isinstance(x, dict):
            return self.layers.get(id(x), "{" + ",".join(sorted(map(str, x))) + "}")
        if isinstance(x, (tuple, list)):
            return "[" + ",".join(self.show(y) for y in x) + "]"
        return repr(x)


T = None  # the trace being written (None: the patches pass everything through)


def patch_torch():
    import torch.distributed as dist

    real_ctx, Stream, Event = torch.cuda.stream, torch.cuda.Stream, torch.cuda.Event
    wait_stream, wait_event, record, record_stream = Stream.wait_stream, Stream.wait_event, Event.record, torch.Tensor.record_stream

    @contextlib.contextmanager
    def stream_ctx(st):
        if T is not None:
            T.log(f"enter {T.stream(st)}")
        with real_ctx(st):
            yield
        if T is not None:
            T.log(f"leave {T.stream(st)}")

    def p_wait_stream(self, other):
        if T is not None:
            T.log(f"wait_stream {T.stream(self)} <- {T.stream(other)}")
        return wait_stream(self, other)

    def p_wait_event(self, ev):
        if T is not None:
            T.log(f"wait_event {T.stream(self)} <- {T.event(ev)}")
        return wait_event(self, ev)

    def p_record(self, stream=None):
        if T is not None:
            T.log(f"record {T.event(self)} on {T.stream(stream if stream is not None else torch.cuda.current_stream())}")
        return record(self, stream) if stream is not None else record(self)

    def p_record_stream(self, st):
        if T is not None:
            T.log(f"record_stream {T.show(self)} on {T.stream(st)}")
        return record_stream(self, st)

    torch.cuda.stream = stream_ctx
    Stream.wait_stream, Stream.wait_event, Event.record, torch.Tensor.record_stream = p_wait_stream, p_wait_event, p_record, p_record_stream

    def gather(name):
        real = getattr(dist, name)

        def patched(out, inp, *a, **kw):
            if T is not None:
                T.log(f"{name} {T.show(inp)}{T.here()}")
            return real(out, inp, *a, **kw)

        setattr(dist, name, patched)

    gather("all_gather")
    gather("all_gather_into_tensor")


def wrap(backend, seen):
    """The backend's entry points, wrapped on the instance (where the tests put their own counters)."""
    for name in ENTRY + ALSO:
        if not hasattr(backend, name):
            continue

        def wrapper(*args, _name=name, _real=getattr(backend, name), **kw):
            seen.add(_name)
            shown = [a.type if isinstance(a, torch.device) else T.show(a) for a in args] + [f"{k}={T.show(v)}" for k, v in kw.items()]
            T.log(f"{_name} {' '.join(shown)}{T.here()}")
            res = _real(*args, **kw)
            if _name == "factorize":
                T.tag(res, T.show(args[0]))
            elif _name == "factorize_many":
                for lay, fac in zip(args[0], res):
                    T.tag(fac, T.show(lay))
            elif _name == "unpack":
                T.tag(res, "U")
            elif _name == "pack":
                T.tag(res, "P")
            return res

        setattr(backend, name, wrapper)


def run(out_dir, name, sdist, backend, streams_of_layers, seen, join=True, after=None):
    """One scenario: every stream of layers twice through quantize_stream on ONE backend (after: the GPU scenarios' fence)."""
    global T
    names = {}
    if after is not None:
        names[torch.cuda.current_stream().cuda_stream] = "caller"
        fs, cs, ls = backend.streams()
        if fs is not None:
            for kind, group in (("f", fs), ("l", ls)):
                for i, st in enumerate(group):
                    names[st.cuda_stream] = f"{kind}{i}"
            names[cs.cuda_stream] = "c"
    T = Trace([lay for layers in streams_of_layers for lay in layers], names)
    wrap(backend, seen)
    try:
        for s, layers in enumerate(streams_of_layers):
            for call in (1, 2):
                T.log(f"== stream {s} call {call} ==")
                shards = sdist.quantize_stream(layers, backend, join=join)
                T.log("returned " + " ".join(f"{sh['rows'][0]}:{sh['rows'][1]}" for sh in shards))
                if after is not None:
                    after()
    finally:
        lines, T = T.lines, None
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{name}: {len(lines)} lines", flush=True)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------- the GPU scenarios (HipBackend)
def gpu_scenarios(out_dir):
    import torch.distributed as dist

    from sleekit_amd import _device as dev
    from sleekit_amd import codebook, synth
    from sleekit_amd import dist as sdist

    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    cb = codebook.UniformCodebook(8, -1, 1)
    seen = set()

    def make(shapes, seed, **extra):
        layers = []
        for i, (R, n) in enumerate(shapes):
            lay = synth.make_layer(R, n, seed + i)
            layers.append(dict({k: torch.from_numpy(lay[k]).to(device) for k in ("W", "H", "scale")}, **extra))
        return layers

    def after():
        torch.cuda.synchronize()
        dev.raise_pending()

    def backend(overlap, moves=0, **attrs):
        be = sdist.HipBackend(cb, "diag", 0.01, moves, with_error=True, overlap=overlap)
        for key, value in attrs.items():
            setattr(be, key, value)
        return be

    # one rank: small layers (batched rounds by shape), short-wide ones (one launch chain, one stacked loop), a small one alone
    # and a tall wide one (the usual route), in model order
    mix = make([(256, 192), (100, 320), (1100, 1600), (48, 172), (128, 1100), (256, 192), (1100, 1600), (100, 320), (2100, 1600),
                (48, 172), (1100, 1600), (256, 192)], 3100)
    for join in (True, False):
        for overlap in ((3, 1), (2, 2), False):
            tag = "x".join(map(str, overlap)) if overlap else "off"
            run(out_dir, f"one_rank_join{int(join)}_{tag}", sdist, backend(overlap), [mix], seen, join, after)
    run(out_dir, "one_rank_moves5", sdist, backend((3, 1), moves=5), [mix], seen, False, after)
    # one rank, full-height layers: stacks of the loop
    tall = make([(128, 544)] * 5, 7700, symmetric=True)
    for ts in (1, 2, 4):
        run(out_dir, f"tall_{ts}", sdist, backend((3, 1), local_batch=1, tall_stack=ts), [tall], seen, False, after)
    # one rank of N, rehearsed
    order = make([(256, 512), (512, 1024), (100, 192), (256, 512), (512, 1024), (100, 192), (256, 320)], 300)
    small = make([(100, 192)] * 7, 900) + [order[0]]
    wide = make([(200, 3200)] * 4, 950)
    ragged = make([(1030, 192)] * 10, 970)
    try:
        for N in (2, 4, 8):
            sdist.rehearse = (0, N)
            todo = [order, small, wide] + ([ragged] if N == 8 else [])
            for on_fs in (True, False):
                be = backend((2, 1) if N >= 4 else (3, 1), rounds_on_factor_streams=on_fs)
                run(out_dir, f"rank_of_{N}_onfs{int(on_fs)}", sdist, be, todo, seen, False, after)
        sdist.rehearse = (1, 4)
        run(out_dir, "rank_1_of_4_joined", sdist, backend((2, 2)), [order, small], seen, True, after)
        sdist.rehearse = (0, 2)
        run(out_dir, "rank_of_2_log", sdist, backend((3, 1), exchange_log=[]), [order, small], seen, False, after)
        run(out_dir, "rank_of_2_moves5", sdist, backend((3, 1), moves=5), [order, small], seen, False, after)
        run(out_dir, "rank_of_2_off", sdist, backend(False), [order, small], seen, True, after)
    finally:
        sdist.rehearse = None
    # the exchange on a single rank: pack, all-gather, unpack
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        sdist.always_exchange = True
        run(out_dir, "always_exchange", sdist, backend((3, 1)), [order], seen, True, after)
        run(out_dir, "always_exchange_log", sdist, backend((2, 2), exchange_log=[]), [order], seen, False, after)
    finally:
        sdist.always_exchange = False
        dist.destroy_process_group()
    missing = [name for name in ENTRY if name not in seen]
    if missing:
        sys.exit(f"stream_trace: no scenario reached {', '.join(missing)}")


# ------------------------------------------------------------------------------------------ the CPU scenarios (stand-in backends)
def _stand_ins(tree):
    spec = importlib.util.spec_from_file_location("_stand_ins", os.path.join(tree, "tests", "test_dist_gloo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cpu_cases(m):
    return [("fake", m.FakeBackend, m.make_layers), ("batch", m.FakeBatchBackend, m.make_equal_layers),
            ("model_order", m.FakeBatchBackend, m.make_model_order_layers), ("status", m.StatusBackend, m.make_layers_with_a_bad_one),
            ("grouping", lambda: m.GroupingBackend(6), m.make_model_order_layers), ("ragged", m.RowsGroupingBackend, m.make_ragged_small_layers)]


def cpu_worker(rank, size, port, tree, out_dir):
    import torch.distributed as dist

    sys.path.insert(0, tree)
    patch_torch()
    from sleekit_amd import dist as sdist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=size)
    try:
        seen = set()
        for name, make_backend, make_layers in cpu_cases(_stand_ins(tree)):
            run(out_dir, f"cpu_world{size}_rank{rank}_{name}", sdist, make_backend(), [make_layers()], seen)
        if size == 1:
            sdist.always_exchange = True
            for name, make_backend, make_layers in cpu_cases(_stand_ins(tree)):
                run(out_dir, f"cpu_always_exchange_{name}", sdist, make_backend(), [make_layers()], seen)
    finally:
        dist.destroy_process_group()


def cpu_scenarios(tree, out_dir):
    import torch.multiprocessing as mp

    from sleekit_amd import dist as sdist

    seen = set()
    m = _stand_ins(tree)
    for name, make_backend, make_layers in cpu_cases(m):
        run(out_dir, f"cpu_one_rank_{name}", sdist, make_backend(), [make_layers()], seen)
        try:
            for rank, N in ((0, 2), (1, 2), (3, 4)):
                sdist.rehearse = (rank, N)
                run(out_dir, f"cpu_rank_{rank}_of_{N}_{name}", sdist, make_backend(), [make_layers()], seen)
        finally:
            sdist.rehearse = None
    ctx = mp.get_context("spawn")
    for size in (2, 1):
        port = _free_port()
        procs = [ctx.Process(target=cpu_worker, args=(r, size, port, tree, out_dir)) for r in range(size)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=120)
            if p.exitcode != 0:
                sys.exit(f"stream_trace: a worker of the {size}-rank world ended with {p.exitcode}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default="stream_traces")
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    tree, out_dir = os.path.abspath(args.tree), os.path.abspath(args.out)
    sys.path.insert(0, tree)
    patch_torch()
    if args.cpu:
        cpu_scenarios(tree, out_dir)
    else:
        gpu_scenarios(out_dir)


if __name__ == "__main__":
    main()
