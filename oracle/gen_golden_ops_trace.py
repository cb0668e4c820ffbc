"""Record what acfe/ops.py hands to the C ABI, launch by launch, over whole
training and inference steps: tests/golden/ops_launch_trace.json.

Test infrastructure only (see oracle/__init__.py).  ops.py never reads a
tensor's values on the host, so its forward and backward run on CPU tensors
when nothing is launched: here `ops.call` is replaced by a recorder
(acfe_conv2d_packed_shape, a host query, is still forwarded to the library;
the `lib.*` queries are untouched), `ops.stream` by a constant and `ops.ptr`
by a wrapper that hands the tensor itself to the recorder.  The fixture pins
every launch ops.py makes -- entry point, scalars, operand shapes and which
buffer goes where -- so that a change of ops.py that is meant to keep
behaviour can be checked exactly, without a GPU (tests/test_ops_trace.py).
Generate it from the tree whose behaviour is the reference -- the commit
BEFORE such a change:

  python oracle/gen_golden_ops_trace.py

Recorded per call, in order: the entry-point name, every scalar argument
(floats by repr), and per pointer argument its shape and dtype (in the row)
and its buffer number by first appearance in the case (beside the row).
Buffers are keyed by data_ptr(); every tensor seen is held until the case ends
so that no address is reused.  None and a tensor without elements are both
null: both reach the C ABI as NULL.  The stream argument is left out.  Cases
marked `ready` also record, in the same sequence, each parameter reported
through ops.set_grad_ready (the bucket order of acfe.dp).

Inference is recorded in bf16 only: an fp32 model runs the same ops.py code
with dtype code 0 (the kernels differ, below the ABI), and the fp32 stem of the
models was not tried this way.

The committed fixture is the recording of commit c0be413, the last one before
the helpers of ops.py were shared.  That tree also had a BN prologue for the
1x1 + BN node behind ACFE_BN_PROLOGUE_C1 (three acfe_c1bn_*_bn entry points);
it was removed with its switch and has no case here.

The fixture is a table: each distinct shape-and-dtype string once (`tensors`),
each distinct row once (`rows`, a pointer argument being [index into
tensors]), and per case the sequence of row indices and the flat sequence of
buffer ages -- how many buffers back the argument's buffer first appeared, 0
for a new one (encode / decode).
"""
import argparse
import contextlib
import itertools
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [p for p in (str(ROOT), str(ROOT / "audio-training_amd")) if p not in sys.path]

CLASSES = 5
# the module switches of ops.py and their default values: every case starts from these
DEFAULTS = dict(FUSE=True, UNPOOL=True, PROLOGUE=True, PRO_POOL=True, PRO_1W=True, FUSE_BN_REDUCE=True,
                STEM_BN_FUSE=True, FUSE_BN_BWD=True, KEEP_BITS=True, FUSE_SUB=True)
SWITCH_GROUPS = {
    "nofuse": dict(FUSE=False, FUSE_BN_REDUCE=False, FUSE_BN_BWD=False, FUSE_SUB=False),
    "noprologue": dict(PROLOGUE=False),
    "nostem_nounpool_nokeep": dict(STEM_BN_FUSE=False, UNPOOL=False, KEEP_BITS=False),
}
BIRD, WRN = (2, 64, 64), (2, 24, 40)  # [N, H, W] of the two models' first cases


class _Stream:
    pass


_STREAM = _Stream()
_DT = {"torch.bfloat16": "bf16", "torch.float32": "f32", "torch.float64": "f64", "torch.uint8": "u8"}


class Recorder:
    """The call sequence of one case: rows (name, args...) and, per row, the
    buffer numbers of its non-null pointer arguments."""

    def __init__(self):
        self.rows, self.bufs, self.alive, self.number = [], [], [], {}

    def call(self, name, *args):
        import torch

        row, bufs = [name], []
        for a in args:
            if a is _STREAM:
                continue
            if isinstance(a, torch.Tensor):
                if a.numel() == 0:
                    row.append(None)
                    continue
                self.alive.append(a)
                bufs.append(self.number.setdefault(a.data_ptr(), len(self.number)))
                row.append(_DT[str(a.dtype)] + json.dumps(list(a.shape), separators=(",", ":")))
            elif a is None or isinstance(a, int):
                row.append(a)
            elif isinstance(a, float):
                row.append(repr(a))
            else:  # a ctypes out-parameter of a host query
                row.append("out")
        self.rows.append(row)
        self.bufs.append(bufs)
        if name == "acfe_conv2d_packed_shape":
            from acfe._lib import call

            return call(name, *args)
        return 0

    def ready(self, names):
        def fn(p):
            self.rows.append(["grad_ready", names[id(p)]])
            self.bufs.append([])
        return fn


@contextlib.contextmanager
def recording(switches=None):
    """ops with the recorder in place of the ABI and the given module switches."""
    from acfe import ops

    rec = Recorder()
    new = dict(DEFAULTS, **(switches or {}))
    new.update(call=rec.call, ptr=lambda t: t, stream=lambda *a: _STREAM, _seed_counter=itertools.count(1),
               _seed_rank=0, _PACK_ACTIVE=None, _PACK_LOG=None, _GRAD_READY=None)
    old = {k: getattr(ops, k) for k in new}
    for k, v in new.items():
        setattr(ops, k, v)
    try:
        yield rec
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def _model(name, shape, train):
    import torch

    if name == "bird":
        from resnet.wr_resnet_bird import WRResNet
    else:
        from resnet.wr_resnet import WRResNet
    # (the layers draw their weights from generators of their own: the global RNG is not touched)
    m = WRResNet(input_shape=(shape[1], shape[2], 3), classes=CLASSES, dtype=torch.bfloat16)
    return m.train(train), torch.zeros(shape, dtype=torch.bfloat16)


def train_step(name, shape, switches=None, arena=True, ready=False, pack=False):
    """forward, loss_and_grad, ParamArena.zero_grad, backward of one model.
    pack: the step records its weight packings as a Trainer's first step does,
    and the WeightPacker built from them packs once."""
    import torch
    from acfe import ops
    from acfe.arena import ParamArena

    with recording(switches) as rec:
        model, x = _model(name, shape, True)
        ar = ParamArena(model, "cpu") if arena else None
        if ready:
            ops.set_grad_ready(rec.ready({id(p): n for n, p in model.named_parameters()}))
        if pack:
            ops._PACK_LOG = []
        z = model(x)
        _, dz = ops.loss_and_grad(z, torch.zeros((shape[0], CLASSES)), "cce")
        if ar is not None:
            ar.zero_grad()
        z.backward(dz)
        if pack:  # the one-launch packer a Trainer builds from its first step
            ops.WeightPacker(ops._PACK_LOG, "cpu").pack()
    return rec


def predict(name, shape):
    import torch

    with recording() as rec, torch.no_grad():
        model, x = _model(name, shape, False)
        model.predict(x)
    return rec


def _t(*shape, dtype=None, grad=False):
    import torch

    return torch.zeros(shape, dtype=dtype or torch.bfloat16, requires_grad=grad)


def op_cast():
    import torch
    from acfe import ops

    with recording() as rec:
        ops.cast(_t(2, 3, 8, dtype=torch.float32), torch.bfloat16)
    return rec


def op_stem_dgrad():
    import torch
    from acfe import ops

    with recording() as rec:
        y, _ = ops.stem_conv(_t(2, 16, 24, grad=True), _t(16, 3, 3, 3, dtype=torch.float32, grad=True),
                             _t(16, dtype=torch.float32, grad=True), torch.bfloat16, want_stats=True)
        y.backward(torch.zeros_like(y))
    return rec


def op_add_relu_untagged():
    import torch
    from acfe import ops

    with recording() as rec:
        z = ops.add(_t(2, 4, 8, 16, grad=True), _t(2, 4, 8, 16, grad=True), relu=True)
        z.backward(torch.zeros_like(z))
    return rec


def op_conv_link_declined():
    import torch
    from acfe import ops

    with recording() as rec:
        x = _t(2, 8, 8, 32, grad=True)[..., :16]
        link = ops.ResidualLink()
        y, _ = ops.conv2d(x, _t(16, 3, 3, 16, dtype=torch.float32, grad=True), _t(16, dtype=torch.float32, grad=True),
                          link=link)
        assert link.declined
        y.backward(torch.zeros_like(y))
    return rec


def op_conv_dropout_bn_odd_height():
    import torch
    from acfe import ops

    f32 = torch.float32
    with recording() as rec:
        y = ops.conv_dropout_bn(_t(2, 7, 16, 64, grad=True), _t(64, 3, 3, 64, dtype=f32, grad=True),
                                _t(64, dtype=f32, grad=True), _t(64, dtype=f32, grad=True),
                                _t(64, dtype=f32, grad=True), _t(64, dtype=f32), _t(64, dtype=f32), True, rate=0.1)
        y.backward(torch.zeros_like(y))
    return rec


def _cases():
    c = [
        # (with the WeightPacker a Trainer builds from its first step's _PACK_LOG, and its pack())
        ("bird_train_2x64x64", lambda: train_step("bird", BIRD, ready=True, pack=True)),
        ("bird_train_2x128x96", lambda: train_step("bird", (2, 128, 96))),
        ("wrn_train_2x24x40", lambda: train_step("wrn", WRN, ready=True)),
        ("wrn_train_2x16x100", lambda: train_step("wrn", (2, 16, 100))),
    ]
    for g, sw in SWITCH_GROUPS.items():
        c.append((f"bird_train_2x64x64_{g}", lambda sw=sw: train_step("bird", BIRD, sw)))
        c.append((f"wrn_train_2x24x40_{g}", lambda sw=sw: train_step("wrn", WRN, sw)))
    c += [
        ("bird_predict_bf16", lambda: predict("bird", BIRD)),
        ("wrn_predict_bf16", lambda: predict("wrn", WRN)),
        ("bird_train_2x64x64_noarena", lambda: train_step("bird", BIRD, arena=False)),
        ("wrn_train_2x24x40_noarena", lambda: train_step("wrn", WRN, arena=False)),
        ("op_cast", op_cast),
        ("op_stem_dgrad", op_stem_dgrad),
        ("op_add_relu_untagged", op_add_relu_untagged),
        ("op_conv_link_declined", op_conv_link_declined),
        ("op_conv_dropout_bn_odd_height", op_conv_dropout_bn_odd_height),
    ]
    return c


CASES = _cases()


def entry_points():
    """The entry-point names ops.py launches (its call("acfe_...") literals):
    the test wants each of them in at least one recorded case."""
    src = (ROOT / "audio-training_amd" / "acfe" / "ops.py").read_text()
    return sorted(set(re.findall(r'\bcall\(\s*"(acfe_[a-z0-9_]+)"', src)))


def record():
    """[(case name, [(row, buffer numbers)])] of the ops.py that is imported."""
    out = []
    for name, run in CASES:
        rec = run()
        out.append((name, list(zip(rec.rows, rec.bufs))))
    return out


def _is_tensor(a):
    return isinstance(a, str) and "[" in a


def encode(cases):
    tensors, rows, trace = {}, {}, {}
    for name, calls in cases:
        idx, ages, newest = [], [], -1
        for row, bufs in calls:
            r = [[tensors.setdefault(a, len(tensors))] if _is_tensor(a) else a for a in row]
            idx.append(rows.setdefault(json.dumps(r, separators=(",", ":")), len(rows)))
            for b in bufs:
                ages.append(newest + 1 - b)
                newest = max(newest, b)
        trace[name] = {"rows": idx, "ages": ages}
    return {"cases": [n for n, _ in cases], "tensors": list(tensors), "rows": [json.loads(k) for k in rows],
            "trace": trace}


def decode(fx):
    """The inverse of encode: [(case name, [(row, buffer numbers)])]."""
    out = []
    for name in fx["cases"]:
        t = fx["trace"][name]
        ages, newest, calls = iter(t["ages"]), -1, []
        for i in t["rows"]:
            row = [fx["tensors"][a[0]] if isinstance(a, list) else a for a in fx["rows"][i]]
            bufs = []
            for a in row:
                if _is_tensor(a):
                    bufs.append(newest + 1 - next(ages))
                    newest = max(newest, bufs[-1])
            calls.append((row, bufs))
        out.append((name, calls))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "ops_launch_trace.json"))
    a = ap.parse_args()
    cases = record()
    fx = encode(cases)
    assert decode(fx) == cases
    Path(a.out).write_text(json.dumps(fx, separators=(",", ":")) + "\n")
    calls = sum(len(t["rows"]) for t in fx["trace"].values())
    print(f"{len(fx['cases'])} cases, {calls} calls, {len(fx['rows'])} distinct rows -> {a.out} "
          f"({Path(a.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
