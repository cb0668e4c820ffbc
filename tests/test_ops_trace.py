"""What acfe/ops.py hands to the C ABI over whole training and inference steps
(every launch: entry point, scalars, operand shapes, which buffer goes where)
against the trace recorded in tests/golden/ops_launch_trace.json
(oracle/gen_golden_ops_trace.py): exact, call by call.  Nothing is launched;
the steps run on CPU tensors and need only the built library."""
import json

from conftest import GOLDEN


def test_ops_launch_trace_matches_the_recording():
    from oracle import gen_golden_ops_trace as gt

    fx = json.loads((GOLDEN / "ops_launch_trace.json").read_text())
    # no case left out: the fixture holds exactly the generator's cases, in order
    assert fx["cases"] == [n for n, _ in gt.CASES]
    want = gt.decode(fx)
    # every entry point ops.py launches (its call("acfe_...") literals) is in at least one recorded case
    reached = {row[0] for _, calls in want for row, _ in calls}
    assert not set(gt.entry_points()) - reached, sorted(set(gt.entry_points()) - reached)

    for (name, exp), (_, got) in zip(want, gt.record()):
        for i, (e, g) in enumerate(zip(exp, got)):
            assert g == e, f"case {name}, call {i}:\n  now      {g[0]} buffers {g[1]}\n  recorded {e[0]} buffers {e[1]}"
        assert len(got) == len(exp), f"case {name}: {len(got)} calls, {len(exp)} recorded"
