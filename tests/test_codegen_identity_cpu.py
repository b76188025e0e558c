"""Generated kernel source is pinned byte for byte: tools/codegen_corpus.py builds its corpus of plans (the kernel catalog,
a matrix over the generator's branches, every switch it reads, plans that fail) through the plan-only entry points and each
text's sha256 and length must equal tests/golden/codegen_digests.json. The text is what csrc/jit.cpp hashes into the code
object's name, so equal text means the same kernels. No GPU needed."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "codegen_digests.json")


@pytest.fixture(scope="module")
def corpus_tool():
    spec = importlib.util.spec_from_file_location("codegen_corpus", os.path.join(ROOT, "tools", "codegen_corpus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_source_is_identical_to_the_golden_digests(corpus_tool):
    with open(GOLDEN) as f:
        want = json.load(f)
    env_before = dict(os.environ)
    got = corpus_tool.digests()
    assert dict(os.environ) == env_before, "the corpus must leave the environment as it found it"
    assert sorted(got) == sorted(want), ("entries only in the corpus: %s; only in the golden file: %s"
                                         % (sorted(set(got) - set(want)), sorted(set(want) - set(got))))
    assert len(want) > 1000
    wrong = [name for name in want if name != "#" and got[name] != want[name]]
    assert not wrong, ("%d of %d entries differ from tests/golden/codegen_digests.json (python tools/codegen_corpus.py --dump DIR writes the texts): %s"
                       % (len(wrong), len(want) - 1, wrong[:20]))


def test_corpus_is_deterministic_and_has_the_catalog(corpus_tool):
    from qurious_amd import catalog
    a, b = corpus_tool.corpus(), corpus_tool.corpus()
    assert a == b
    names = ["catalog: " + name for name, _ in catalog.catalog_sources()]
    assert len(names) == 49 and all(n in a for n in names)
    assert all(not a[n].startswith("ERROR ") for n in names)
