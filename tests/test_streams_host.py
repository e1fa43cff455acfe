"""The stream tests reach every entry point that the write-bounds tests name, and their exceptions are the headers'.  Needs no GPU:
the entry points of the bounds modules (tests/test_bounds_*_gpu.py) are read from their source, the names their test functions pass
to bounds.run / bounds.run_outputs as `what`; those of the stream modules (tests/test_streams_*_gpu.py) from their CATALOGUE, whose
third column the GPU tests hold against the `what` of the cases really reached (streams.check_catalogue).  The GPU modules are
imported for their tables only; importing them builds nothing that is not built and touches no device.
"""
import ast
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PAIRS = {"flow": ("test_bounds_flow_gpu", "test_streams_flow_gpu"), "metrics": ("test_bounds_metrics_gpu", "test_streams_metrics_gpu"),
         "models": ("test_bounds_models_gpu", "test_streams_models_gpu")}
NAME = re.compile(r"\b(?:rnvp|cvae|pfm|pfw|pfn|pfg|pfp)_[a-z][a-z0-9_]*")
EPOCH_WHAT = "rnvp_%s[%s]"               # test_bounds_flow_gpu.test_fit_epoch_calls forms its names from its `entry` argument


def params(fn, name):
    """the values a test function is parametrised with for one argument"""
    found = [list(m.args[1]) for m in getattr(fn, "pytestmark", []) if m.name == "parametrize" and m.args[0] == name]
    assert len(found) == 1, (fn.__name__, name)
    return found[0]


def named_by(module):
    """{test function: the entry points named in the string literals of its body}"""
    import importlib
    mod = importlib.import_module(module)
    tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
    out = {}
    for node in tree.body:
        if not (isinstance(node, ast.FunctionDef) and node.name.startswith("test_")):
            continue
        body = node.body[1:] if ast.get_docstring(node) else node.body
        names = set()
        for stmt in body:
            for sub in ast.walk(stmt):
                if isinstance(sub, ast.Constant) and isinstance(sub.value, str):
                    if sub.value == EPOCH_WHAT:
                        names |= {"rnvp_" + e for e in params(getattr(mod, node.name), "entry")}
                    names |= set(NAME.findall(sub.value))
        if names:
            out[node.name] = names
    return out


def _modules(which):
    import importlib
    b, s = PAIRS[which]
    return importlib.import_module(b), importlib.import_module(s)


def test_the_reader_finds_the_names_the_bounds_modules_pass():
    flow = named_by("test_bounds_flow_gpu")
    assert flow["test_flow_calls"] == {"rnvp_forward_logprob", "rnvp_inverse", "rnvp_sample"}
    assert flow["test_fit_epoch_calls"] == {"rnvp_fit_epoch", "rnvp_fit_epochs", "rnvp_fit_epoch_dp", "rnvp_fit_epoch_dp_cb", "rnvp_fit_epoch_dp_cb_chunked"}
    metrics = named_by("test_bounds_metrics_gpu")
    assert metrics["test_slice_grad"] == {"pfm_slice_grad"} and metrics["test_project"] == {"pfm_project"}
    models = named_by("test_bounds_models_gpu")
    assert models["test_cvae_calls"] == {"cvae_encode", "cvae_decode", "cvae_loss_grad", "cvae_train_step"}
    assert models["test_flow_draw_accumulate"] == {"pfp_draw_accumulate"}
    total = set().union(*flow.values(), *metrics.values(), *models.values())
    assert len(total) >= 50, sorted(total)


@pytest.mark.parametrize("which", list(PAIRS))
def test_every_entry_point_of_the_bounds_catalogue_is_reached_by_a_stream_case(which):
    bmod, smod = _modules(which)
    named = named_by(PAIRS[which][0])
    reached = {}
    for test, kwargs, expect in smod.CATALOGUE:
        fn = getattr(bmod, test)                                 # the case runs a test function of the bounds module, with its arguments
        assert set(kwargs) == set(inspect.signature(fn).parameters), (test, kwargs)
        assert set(expect) <= named[test], (test, expect)
        reached.setdefault(test, set()).update(expect)
    for test, names in named.items():
        if test.startswith("test_the_detector"):                 # the bounds driver's own self-test calls the library directly
            continue
        missing = names - reached.get(test, set())
        assert not missing, "%s: no stream case reaches %s through %s" % (PAIRS[which][1], sorted(missing), test)


def test_the_entry_points_outside_the_bounds_catalogue_have_cases_of_their_own():
    _, smod = _modules("flow")
    header = open(os.path.join(ROOT, "include", "rnvp_hip.h")).read()
    source = open(os.path.join(ROOT, "tests", "test_streams_flow_gpu.py")).read()
    assert set(smod.ADDED) == {"rnvp_adam_step", "rnvp_dp_finish_step", "rnvp_prior_normal"}
    for name in smod.ADDED:
        assert re.search(r"int %s\(void \*stream," % name, header), name
        assert 'streams.run("%s[' % name in source, name


def test_every_exception_quotes_its_header():
    """the sentence of an exception is `<header's path under probaforms_amd>: piece ... piece`, every piece in the header word for word"""
    _, smod = _modules("models")
    for entry, form, sentence, still in smod.EXCEPTIONS:
        path, quoted = sentence.split(": ", 1)
        text = open(os.path.join(ROOT, "probaforms_amd", path)).read()
        assert re.search(r"int\s+%s\(void \*stream," % entry, text), entry
        header = " ".join(text.replace("\n * ", " ").split())
        for piece in quoted.split(" ... "):
            assert piece in header, (entry, piece)
        assert smod.waits("%s[lmm, 19 draws, %s]" % (entry, form)) == sentence and smod.waits("%s[lmm, 19 draws, z given]" % entry) is None
    for which in ("flow", "metrics"):
        assert not hasattr(_modules(which)[1], "EXCEPTIONS")
