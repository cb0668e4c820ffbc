"""The host-only dispatch queries of the convolution launchers (no GPU call)
against the answers recorded in tests/golden/conv_dispatch_plan.json
(oracle/gen_golden_dispatch.py): every query of every shape of the grid, exact."""
import json
import os

from conftest import GOLDEN


def test_dispatch_answers_match_the_recorded_plan():
    from oracle import gen_golden_dispatch as gd

    # the fixture is the default configuration's: a dispatch switch changes the answers
    set_ = [n for n in gd.dispatch_switches() if n in os.environ]
    assert not set_, f"dispatch switches set in the environment: {set_}"

    from acfe._lib import lib

    want = json.loads((GOLDEN / "conv_dispatch_plan.json").read_text())
    assert want["shape_queries"] == list(gd.SHAPE_QUERIES)
    # no entry left out: the fixture holds exactly the generator's grid, in its order
    assert [tuple(e[:5]) for e in want["shapes"]] == gd.SHAPES
    assert [tuple(e[:3]) for e in want["stem_blocks"]] == gd.IMAGES
    assert [tuple(e[:2]) for e in want["packed_shape"]] == gd.CHANNELS

    bad = []
    for e in want["shapes"]:
        shape, exp = tuple(e[:5]), e[5:]
        got = gd.shape_answers(lib, *shape)
        assert len(got) == len(exp) == len(gd.SHAPE_QUERIES)
        bad += [f"{q} (N, H, W, C, K) = {shape}: {g} != recorded {x}"
                for q, g, x in zip(gd.SHAPE_QUERIES, got, exp) if g != x]
    for *image, exp in want["stem_blocks"]:
        got = gd.image_answer(lib, *image)
        if got != exp:
            bad.append(f"acfe_stem_blocks (N, H, W) = {tuple(image)}: {got} != recorded {exp}")
    for e in want["packed_shape"]:
        got = gd.channel_answer(lib, *e[:2])
        if got != e[2:]:
            bad.append(f"acfe_conv2d_packed_shape (C, K) = {tuple(e[:2])}: {got} != recorded {e[2:]}")
    assert not bad, f"{len(bad)} answers differ:\n" + "\n".join(bad[:40])
