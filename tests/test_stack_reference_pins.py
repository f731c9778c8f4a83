"""Regression pins of the image-stack consumers' host references (tests/golden/stack_reference_pins.json, written by oracle/make_stack_pins.py): SHA-256 of what the
eight fuse and accumulate references and the four record makers give on the inputs of the six tests/*_cases.py modules.  The kernels are held to the references bit
for bit, and the references to float64 readings within a tolerance: these digests hold the references' own bits, so that a header shared by both cannot drift by an
ulp unseen.  The GPU test holds every *_images call to the same digests; with the *_views-equals-*_images tests of the other files that pins the context calls too."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pins_module():
    spec = importlib.util.spec_from_file_location("make_stack_pins", os.path.join(ROOT, "oracle", "make_stack_pins.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "stack_reference_pins.json")))


def test_references_reproduce_their_pins(pkg):
    got = _pins_module().compute()
    assert got.keys() == PINS.keys()
    wrong = sorted(k for k in PINS if got[k] != PINS[k])
    assert not wrong, wrong


@pytest.mark.gpu
def test_images_calls_reproduce_the_pins(ctx, pkg):
    got = _pins_module().compute(ctx)
    assert got and got.keys() <= PINS.keys()
    assert {k.split("/")[0] for k in got} == {"%s_reference%s" % (a, b) for a in ("fuse", "accumulate") for b in ("", "_frames", "_motion", "_deform")}
    wrong = sorted(k for k in got if got[k] != PINS[k])
    assert not wrong, wrong
