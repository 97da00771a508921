"""The ORDER and the arguments of everything engine.Net and the wgan step enqueue, held on the CPU.

tests/golden/make_engine_trace.py replaces the launches (``ops``) and the collectives (``dist``) by recorders and runs a set of
tiny configurations; tests/golden/engine_trace.json is what the engine enqueued for them when the fixture was made.  A change of
the engine that is meant to leave its launch list alone (a refactor) must reproduce the file; one that is meant to change it
reruns the maker and shows the difference in review.

Whole ``train_on_batch`` calls run under the stubs (``step_replay=False``, models built on the CPU, optimizer launches
recorded like the rest).  Left out: step programs (recording needs the device), the ``capture_branches`` instrumentation, and
torch-side host plumbing (tap upload, the metric buffer's read)."""
import importlib.util
import json
import os

import pytest

import blurred_gan_amd as bg
from blurred_gan_amd import engine  # noqa: F401  (bg.engine)

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_engine_trace", os.path.join(HERE, "golden", "make_engine_trace.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

COVERS = "\n".join(f"  {name} -> {what}" for name, (what, _, _) in maker.CONFIGS.items())


@pytest.fixture(scope="module")
def fixture():
    maker.ensure_library(os.path.dirname(HERE))          # the host queries (workspace sizes, blur policy) are the library's own
    with open(maker.FIXTURE) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_the_configurations(fixture):
    assert sorted(fixture) == sorted(maker.CONFIGS)


@pytest.mark.parametrize("name", sorted(maker.CONFIGS))
def test_the_engine_enqueues_what_the_fixture_holds(fixture, name):
    got, want = maker.run_config(bg, name), fixture[name]
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f"{name}: call {n} differs\n  engine : {g}\n  fixture: {w}\n  after  : {got[n - 1] if n else '(first call)'}\n"
                        f"configuration -> branches it reaches:\n{COVERS}")
    assert len(got) == len(want), (f"{name}: {len(got)} calls, the fixture holds {len(want)}; first surplus call: "
                                   f"{(got + want)[min(len(got), len(want))]}\nconfiguration -> branches it reaches:\n{COVERS}")


def test_rerunning_the_maker_reproduces_the_file_byte_for_byte(fixture):
    with open(maker.FIXTURE) as fh:
        assert maker.dumps(maker.make(bg)) == fh.read()


def test_the_configurations_execute_every_line_of_the_four_passes(fixture):
    """Every line of Net.forward / backward / gp_second_order / gp_second_order_merged is run by at least one configuration
    (only the capture_branches instrumentation is left out), so no branch of them can change its launches unseen."""
    missed = maker.missed_lines(bg)
    assert not missed, f"engine.py lines no configuration executes: {missed}\nconfiguration -> branches it reaches:\n{COVERS}"
