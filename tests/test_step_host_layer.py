"""The host layer of the composed step (bench_step.py): the sections are named once, a choice is an argument, the
command line becomes keywords in one function, the training loop is written once.  The table of switches against what reaches ``Step`` and the
harnesses, and a source scan of the same shape as tests/test_loss_host_layer.py; no GPU.

``SECTIONS`` names a section; its method is ``Step.<name>_section``, because four of the seven bare names (backbone, input_proj, encoder,
decoder) are sub-modules of ``Step`` whose names are the state dict's keys, which the tests and tools of the tree read."""
import os
import re

import pytest

import bench_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("backbone", "input_proj", "encoder", "two_stage", "dn", "decoder", "heads")
# flag -> (the keyword it sets, who receives it)
FLAGS = {"--fed-loss": ("fed_loss", "step"), "--device-distill": ("device_distill", "step"), "--device-dn": ("device_dn", "step"),
         "--device-geometry": ("device_geometry", "step"), "--library-optimizer": ("library", "harness"),
         "--grouped-repack": ("grouped_repack", "harness")}
OFFERED = ("Step", "run", "run_graphed", "run_graphed_device", "run_ddp", "make_optimizer", "optimizer_step", "GroupedRepack",
           "pin_grad_accumulators", "box_cxcywh_to_xyxy", "giou_pairs", "sine_position", "encoder_output_proposals", "inverse_sigmoid",
           "synthetic_image_counts", "LR", "CLIP_MAX_NORM", "NUM_CLASSES", "NUM_QUERIES", "DN_NUMBER")


def _kwargs(argv):
    return bench_step.cli_kwargs(bench_step.parse_args(argv))


def _expected(flags, boxes=12):
    step, harness = {"boxes_per_image": boxes}, {"steps": 5, "warmup": 2}
    for f in flags:
        kw, who = FLAGS[f]
        (step if who == "step" else harness)[kw] = True
    return step, harness


def test_the_table_is_the_command_line():
    assert {(flag, kw) for flag, kw, _ in bench_step.SWITCHES} == {(f, kw) for f, (kw, _) in FLAGS.items()}
    assert all(text for _, _, text in bench_step.SWITCHES)


@pytest.mark.parametrize("flags", [()] + [(f,) for f in FLAGS] + [tuple(FLAGS)], ids=lambda f: "+".join(f) or "none")
def test_flags_become_exactly_their_keywords(flags):
    assert _kwargs(list(flags)) == _expected(flags)


def test_boxes_per_image_arrives_and_defaults_to_12():
    assert _kwargs(["--boxes-per-image", "7"]) == _expected((), boxes=7)
    assert _kwargs(["--boxes-per-image", "7", "--device-dn", "--steps", "3", "--warmup", "1"]) == \
        ({"boxes_per_image": 7, "device_dn": True}, {"steps": 3, "warmup": 1})
    assert bench_step.parse_args([]).boxes_per_image == 12


def test_step_keywords_are_keywords_of_step_and_harness_keywords_of_every_harness():
    import inspect
    step, harness = _kwargs(list(FLAGS))
    assert set(step) <= set(inspect.signature(bench_step.Step.__init__).parameters)
    for fn in (bench_step.run, bench_step.run_graphed, bench_step.run_graphed_device):
        assert set(harness) <= set(inspect.signature(fn).parameters), fn.__name__


def _main_with_recorded_harnesses(monkeypatch, argv):
    calls = []

    def record(name):
        def fn(n_img, dev, **kw):
            calls.append((name, n_img, kw))
            return {"ms": 1.0, "img_per_s": 2.0, "loss": 3.0}
        return fn
    monkeypatch.setattr(bench_step, "run", record("run"))
    monkeypatch.setattr(bench_step, "run_graphed", record("run_graphed"))
    monkeypatch.setattr(bench_step.torch.cuda, "empty_cache", lambda: None)
    bench_step.main(argv)
    return calls


def test_device_matcher_selects_the_three_run_branch(monkeypatch, capsys):
    calls = _main_with_recorded_harnesses(monkeypatch, ["--device-matcher", "--fed-loss", "--grouped-repack", "--boxes-per-image", "7"])
    want = {"steps": 5, "warmup": 2, "grouped_repack": True, "boxes_per_image": 7, "fed_loss": True}
    assert calls == [("run_graphed", 2, {"device_matcher": dm, **want}) for dm in (False, False, True)]
    assert '"device_matcher"' in capsys.readouterr().out


def test_without_it_the_one_run_branch(monkeypatch, capsys):
    calls = _main_with_recorded_harnesses(monkeypatch, ["--stop-at", "encoder", "--device-geometry", "--library-optimizer"])
    assert calls == [("run", 2, {"graph": False, "stop_at": "encoder", "steps": 5, "warmup": 2, "library": True, "boxes_per_image": 12,
                                 "device_geometry": True})]
    calls = _main_with_recorded_harnesses(monkeypatch, [])
    assert calls[-1] == ("run", 2, {"graph": True, "stop_at": None, "steps": 5, "warmup": 2, "boxes_per_image": 12})
    capsys.readouterr()


def test_sections_are_named_once(capsys):
    assert bench_step.SECTIONS == NAMES
    for name in NAMES:
        assert callable(getattr(bench_step.Step, name + "_section")), name
    with pytest.raises(SystemExit):
        bench_step.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--stop-at" in text and ", ".join(NAMES) in text


def test_offered_names():
    missing = [n for n in OFFERED if not hasattr(bench_step, n)]
    assert not missing, missing


# ---- source scan -----------------------------------------------------------------------------------------------------------------------------
def _python_files():
    for top in ("", "richsem_amd", "tests", "tools"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if not x.startswith(".") and x != "__pycache__"] if top else []
            yield from (os.path.join(d, f) for f in files if f.endswith(".py"))


def _function_source(text, name):
    m = re.search(r"^def %s\(.*?(?=^(?:def|class) |\Z)" % name, text, re.M | re.S)
    assert m, name
    return m.group(0)


def test_the_choice_no_longer_travels_through_an_attribute():
    word = "_model" + "_only"      # (spelled in two parts: this file is read too)
    hits = [os.path.relpath(p, ROOT) for p in _python_files() if word in open(p, encoding="utf-8").read()]
    assert hits == [], hits


def test_the_loop_and_the_weight_decay_are_written_once():
    text = open(os.path.join(ROOT, "bench_step.py"), encoding="utf-8").read()
    call = ".backward" + "()"
    for name in ("run", "run_graphed", "run_graphed_device"):
        lines = [ln for ln in _function_source(text, name).splitlines() if call in ln]
        assert len(lines) <= 1, (name, lines)
        assert all("eager once" in ln for ln in lines), (name, lines)      # the warm-up pass; the loop helper holds the other
    assert _function_source(text, "run").count(call) == 0
    assert text.count("weight_decay" + "=") == 1
