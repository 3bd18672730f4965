"""The caller-stream contract of include/dcv.h on the MI355X: every entry of tests/stream_cases.py on a side stream with
work pending in front of it.

The float64 oracle tests run every kernel on the default stream with nothing pending, where a launch, memset or copy on
the wrong stream, a synchronisation of the wrong stream or a host array read too late still gives correct numbers.
Here each case runs

  reference        twice on the default stream with clean inputs (this also warms every lazy allocation).  Outputs
                   whose two runs agree in bits are compared bit for bit below; outputs that differ (float atomics) at
                   the tolerance of the entry's own oracle test, and the case is reported as not deterministic;
  warm             once on the side stream with nothing pending (also fills the side stream's pool of torch's allocator,
                   so that no later run allocates);
  pending          on the side stream: device inputs allocated as poison, a delay kernel, an event `gate`, the clean
                   inputs copied in, then the call.  Whatever the entry runs off the side stream runs during the delay,
                   reads poison, and the comparison fails.  A step without host arrays and host outputs must return
                   while the gate is still closed -- if it is open the run has shown nothing and the test FAILS saying
                   so (after retrying once with a longer delay);
  released         the same, and the moment a step returns every host array the case lists is overwritten with valid but
                   wrong values; behind the last step the device inputs are poisoned again on the side stream;
  two streams      two different cases on two side streams, each behind its own delay, let go together.

Five entries are called without their wrapper (tests/stream_cases.py says how): hip.dip_sorted, hip.linkage,
hip.core_distances and hip.mr_mst read the input back before they call the library, and hip.xtc_encode reads the
descriptors back between its two entries, so behind the wrapper the stream would be idle when the entry runs.

Poison never turns into an address: floats are NaN (zeros where finite input is the entry's precondition), indices,
labels and bytes are zeros.  What the probes cannot see: the library's local std::vector copies of host arrays (only the
caller's own arrays can be overwritten at return); state built lazily by the first call of an engine (the reference
runs build it); host threads calling concurrently; the read-backs of the five wrappers that are bypassed.  At most three streams exist here: the default one and two from
torch.cuda.Stream().  DESIGN.md (the caller-stream contract) holds the measured gate table."""
import os

import numpy as np
import pytest
import torch

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu

DELAYS_MS = (20.0, 160.0)     # the delay in front of a segment; the second is tried once when an asynchronous step found the gate open
_SIDE = []                    # the two side streams of this module
_START_MODE = []              # the arithmetic mode of the process when the module began
_PREPARED = {}                # (case name, flavour) -> Prepared: clean inputs on the device, engine, reference outputs
GATE_ROWS = []                # (case, flavour, probe, step, may block, returned with the gate closed)
NOT_DETERMINISTIC = set()     # (case, flavour, output) whose two default-stream runs differed in bits


def side(i):
    while len(_SIDE) <= i:
        assert len(_SIDE) < 2, "this module opens two side streams and no more"
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[i]


# ------------------------------------------------------------------------------------------------ the delay
@pytest.fixture(scope="module")
def delay():
    """delay(ms): enqueue about `ms` milliseconds of device time on the current stream.  torch.cuda._sleep counts device
    clock ticks; ticks per millisecond are measured once with events.  Should the kernel not run on the device, a chain of
    dependent torch.mm sized by the same measurement stands in."""
    s = side(0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            fn()   # first launch: code object load
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    per_ms = None
    try:
        for ticks in (1_000_000, 50_000_000):
            ms = timed(lambda: torch.cuda._sleep(ticks))
            if ms >= 2.0:
                per_ms = ticks / ms
                break
    except (AttributeError, RuntimeError):
        per_ms = None
    if per_ms is not None:
        print(f"delay: torch.cuda._sleep, {per_ms:.0f} ticks per millisecond")
        yield lambda ms: torch.cuda._sleep(int(per_ms * ms))
    else:
        x = torch.full((1024, 1024), 1.0 / 1024, device="cuda")

        def chain(n):
            y = x
            for _ in range(n):
                y = torch.mm(y, x)
        links_per_ms = 64 / timed(lambda: chain(64))
        print(f"delay: chain of dependent 1024^3 products, {links_per_ms:.1f} per millisecond")
        yield lambda ms: chain(max(1, int(links_per_ms * ms)))
    _report()


def test_the_delay_holds_the_gate(delay):
    s = side(0)
    a, gate = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record()
        delay(DELAYS_MS[0])
        gate.record()
    closed = not gate.query()
    gate.synchronize()
    ms = a.elapsed_time(gate)
    print(f"a {DELAYS_MS[0]} ms delay took {ms:.2f} ms")
    assert closed, "the gate was open right after the delay was enqueued: the delay kernel does not hold the stream"
    assert 0.5 * DELAYS_MS[0] <= ms <= 4 * DELAYS_MS[0], ms


# ------------------------------------------------------------------------------------------------ running a case
class Prepared:
    def __init__(self, case, flavour):
        from deep_cartograph_amd import hip

        self.case, self.flavour, self.hip = case, flavour, hip
        dev, self.host = case.build()
        self.clean = {k: torch.from_numpy(v).cuda() for k, v in dev.items()}
        self.poison = {k: case.poison.get(k, sc.default_poison(v)) for k, v in dev.items()}
        self.mode()
        self.eng = case.engine(hip) if case.engine else None
        torch.cuda.synchronize()
        first, second = self.on_default_stream(), self.on_default_stream()
        assert first.keys() == second.keys()
        self.reference = first
        self.loose = {k for k in first if not same_bits(first[k], second[k])}
        for k in sorted(self.loose):
            NOT_DETERMINISTIC.add((case.name, flavour or "", k))
            assert case.tolerance is not None, f"{case.name}: output {k} differs between two default-stream runs and the case names no tolerance"
            close(second[k], first[k], case.tolerance, f"{case.name}: {k}, second default-stream run")

    def mode(self):
        """The arithmetic mode is process-wide host state read at every call: set before each step, also for a case that
        names no flavour (it runs in the mode the module started in), because two cases take turns in the two-stream probe."""
        self.hip.set_gemm_mode(self.flavour or _START_MODE[0])

    def segments(self, tensors, host):
        args = (self.hip, tensors, host) + ((self.eng,) if self.eng is not None else ())
        return self.case.steps(*args)

    def on_default_stream(self):
        tensors = {k: v.clone() for k, v in self.clean.items()}
        out = {}
        for seg in self.segments(tensors, {k: v.copy() for k, v in self.host.items()}):
            for step in seg:
                self.mode()
                collect(out, step, step.fn(), tensors)
        torch.cuda.synchronize()
        return to_host(out)

    def close(self):
        if self.eng is not None:
            self.eng.close()


def prepared(case, flavour):
    key = (case.name, flavour)
    if not _START_MODE:
        from deep_cartograph_amd import hip

        _START_MODE.append(hip.get_gemm_mode())
    if key not in _PREPARED:
        _PREPARED[key] = Prepared(case, flavour)
    return _PREPARED[key]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    from deep_cartograph_amd import hip

    start = hip.get_gemm_mode()
    yield
    hip.set_gemm_mode(start)
    _START_MODE.clear()
    for p in _PREPARED.values():
        p.close()
    _PREPARED.clear()


def collect(out, step, got, tensors):
    """Outputs of a step under '<step>.<name>'; one that IS an input tensor (labels, running minima) is copied, in stream
    order, because the probes poison the inputs afterwards."""
    for k, v in (got or {}).items():
        if isinstance(v, torch.Tensor) and any(v is t for t in tensors.values()):
            v = v.clone()
        out[f"{step.name}.{k}"] = v


def to_host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def close(got, ref, tolerance, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if np.issubdtype(ref.dtype, np.floating):
        np.testing.assert_allclose(got, ref, rtol=tolerance[0], atol=tolerance[1], equal_nan=True, err_msg=what)
    else:
        assert np.array_equal(got, ref), what


def fill(t, kind):
    if kind == "nan":
        t.fill_(float("nan"))
    else:
        t.zero_()


def probe(items, probe_name, delay, delay_ms):
    """Run the prepared cases `items`, item i on side stream i, segment by segment and step by step in turn.  Returns
    (outputs per item, [step names that had to return with the gate closed and did not] per item)."""
    streams = [side(i) for i in range(len(items))]
    pending = probe_name != "warm"
    tensors, hosts, segs, outs, opened = [], [], [], [], []
    for it, s in zip(items, streams):
        with torch.cuda.stream(s):   # 1. the device inputs, allocated as poison
            t = {k: torch.empty_like(v) for k, v in it.clean.items()}
            for k in t:
                fill(t[k], it.poison[k])
        host = {k: v.copy() for k, v in it.host.items()}
        tensors.append(t)
        hosts.append(host)
        segs.append(it.segments(t, host))
        outs.append({})
        opened.append([])
    for g in range(max(len(sg) for sg in segs)):
        gates = []
        for it, s, t, sg in zip(items, streams, tensors, segs):
            gate = torch.cuda.Event()
            gates.append(gate)
            if g >= len(sg):
                continue
            with torch.cuda.stream(s):
                if g > 0:
                    for k in t:
                        fill(t[k], it.poison[k])
                if pending:
                    delay(delay_ms)          # 2. the delay
                gate.record()                # 3. the gate
                for k in t:                  # 4. the clean inputs
                    t[k].copy_(it.clean[k], non_blocking=True)
        todo = [list(sg[g]) if g < len(sg) else [] for sg in segs]
        # Judging the gate.  Inside one case no asynchronous step follows a step that may hold the host (checked without a GPU
        # by tests/test_stream_cases_cpu.py), so with one case on one stream EVERY asynchronous step is judged.  With two
        # cases the streams take turns and the asynchronous steps of both go first; `held` only waives the gate for what is
        # left of one engine's asynchronous steps when the other engine's sequence was shorter and has reached its read_log
        # (which waits out both delays).  Those steps are still compared, and each was judged in its own single-case test.
        held = False

        def run(i):
            it, step = items[i], todo[i].pop(0)
            it.mode()
            with torch.cuda.stream(streams[i]):
                got = step.fn()              # 5. the call
                closed = not gates[i].query()
                collect(outs[i], step, got, tensors[i])
            if probe_name == "released":
                for k in it.case.host_arrays:
                    hosts[i][k][...] = np.zeros((), dtype=hosts[i][k].dtype) if k not in it.case.scribble else it.case.scribble[k]
            if pending:
                GATE_ROWS.append((it.case.name, it.flavour or "", probe_name, step.name, step.blocks or "", closed, held and not step.blocks))
                if not held and not step.blocks and not closed:
                    opened[i].append(step.name)

        while any(todo):
            # the asynchronous steps first, the streams taking turns; only when every stream's next step may hold the host
            # does one run
            while any(t and not t[0].blocks for t in todo):
                for i, t in enumerate(todo):
                    if t and not t[0].blocks:
                        run(i)
            for i, t in enumerate(todo):
                if t:
                    run(i)
                    held = True
    if probe_name == "released":
        for it, s, t in zip(items, streams, tensors):
            with torch.cuda.stream(s):
                for k in t:
                    fill(t[k], it.poison[k])
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    return [to_host(o) for o in outs], opened


def check(it, got, what):
    ref = it.reference
    assert got.keys() == ref.keys(), what
    for k in ref:
        if k in it.loose:
            close(got[k], ref[k], it.case.tolerance, f"{what}: {k}")
        else:
            assert same_bits(got[k], ref[k]), (f"{what}: output {k} differs in bits from the default-stream reference "
                                                f"({_differences(got[k], ref[k])})")


def _differences(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{a.dtype}{a.shape} against {b.dtype}{b.shape}"
    bad = np.ascontiguousarray(a).view(np.uint8).reshape(a.size, -1) != np.ascontiguousarray(b).view(np.uint8).reshape(b.size, -1) if a.size else np.zeros((0, 1), bool)
    n = int(bad.any(axis=1).sum())
    nan = int(np.isnan(a).sum()) if np.issubdtype(a.dtype, np.floating) else 0
    return f"{n} of {a.size} elements, {nan} NaN"


def run_behind_pending_work(items, probe_name, delay, what):
    """The probe with the 20 ms delay; once more with the long one if an asynchronous step found the gate open.  Every
    run is compared; an open gate at the long delay fails the test: such a run has shown nothing."""
    for delay_ms in DELAYS_MS:
        got, opened = probe(items, probe_name, delay, delay_ms)
        for it, g in zip(items, got):
            check(it, g, f"{it.case.name} [{it.flavour}] {what}, {delay_ms:.0f} ms delay")
        if not any(opened):
            return
    raise AssertionError(f"{what}: {[(it.case.name, o) for it, o in zip(items, opened) if o]} take no host array and have no host "
                         f"output, yet returned with the gate open behind a {DELAYS_MS[-1]:.0f} ms delay: the call waited for the "
                         f"stream, and the run has shown nothing about its ordering")


SINGLE = [(c, f) for c in sc.CASES for f in c.flavours]


@pytest.mark.parametrize("case,flavour", SINGLE, ids=[f"{c.name}-{f}" if f else c.name for c, f in SINGLE])
def test_entry_behind_pending_work_and_with_inputs_released(case, flavour, delay):
    it = prepared(case, flavour)
    got, _ = probe([it], "warm", delay, 0.0)
    check(it, got[0], f"{case.name} on an idle side stream")
    run_behind_pending_work([it], "pending", delay, "behind pending work")
    run_behind_pending_work([it], "released", delay, "with its inputs released at return")


def _pairs():
    """Every stateless case with its neighbour in the table, and the engines two by two (two separate hip.Mlp handles)."""
    table = [c for c in sc.CASES if c.stateless]
    pairs = [(table[i], table[(i + 1) % len(table)]) for i in range(0, len(table), 2)]
    eng = {c.name: c for c in sc.CASES if c.engine}
    pairs += [(eng["mlp deep_tica block"], eng["mlp ae fused"]), (eng["mlp ae block"], eng["mlp deep_tica fused"]),
              (eng["mlp vae dropout"], eng["mlp deep_tica block"]), (eng["mlp vae fused"], eng["mlp deep_tica batchnorm"])]
    return pairs


PAIRS = _pairs()


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a.name}+{b.name}" for a, b in PAIRS])
def test_two_cases_on_two_streams_at_once(a, b, delay):
    items = [prepared(a, a.flavours[0]), prepared(b, b.flavours[-1] if a.engine and b.engine else b.flavours[0])]
    got, _ = probe(items, "warm", delay, 0.0)
    for it, g in zip(items, got):
        check(it, g, f"{it.case.name} on an idle side stream next to {[x.case.name for x in items if x is not it][0]}")
    run_behind_pending_work(items, "two streams", delay, f"{a.name} and {b.name} on two streams at once")


# ------------------------------------------------------------------------------------------------ the measured table
def _report():
    """The gate table and the outputs compared by tolerance, printed at the end of the module and, with
    DCV_STREAM_GATE_TABLE=<path>, written there (DESIGN.md quotes it)."""
    rows = {}
    for case, flavour, probe_name, step, blocks, closed, behind in GATE_ROWS:
        key = (case, flavour, step)
        r = rows.setdefault(key, {"blocks": blocks, "closed": 0, "open": 0, "behind": behind})
        r["closed" if closed else "open"] += 1
    lines = ["case | flavour | step | may hold the host because | returned with the gate closed / open"]
    for (case, flavour, step), r in rows.items():
        why = r["blocks"] or ("(behind a step that may)" if r["behind"] else "")
        lines.append(f"{case} | {flavour} | {step} | {why} | {r['closed']} / {r['open']}")
    lines.append("")
    lines.append("outputs compared by tolerance (two default-stream runs differ in bits): " +
                 (", ".join(f"{c} [{f}] {k}" for c, f, k in sorted(NOT_DETERMINISTIC)) or "none"))
    text = "\n".join(lines)
    print(text)
    path = os.environ.get("DCV_STREAM_GATE_TABLE")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
