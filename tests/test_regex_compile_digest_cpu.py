"""The -E compilers answer as they did before their rules were folded into one copy each (host only): tools/regex_compile_san.cpp
--digest asks the compilers and regex_compile_search about a fixed corpus and prints one FNV-1a digest per 1000 entries of
their answers (taken or refused, every byte of a taken struct, the reason of a refusal); tests/golden/regex_compile_digest.json is
what the compilers of the commit before said (the tool's head names the command that reproduces it).  The rows without a dot are the
four older compilers'; loops.*, groups.*, search10.*, search01.*, search11.* and walk.* are the loops and the groups compiler, the
search order with their switches on, and the line walk program of everything they take.  Here: every named table and the first 20
blocks of each random corpus; `python tools/sanitize.py regex` compares the whole corpus."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = 20
NEW_ROWS = ("loops", "groups", "search10", "search01", "search11", "walk")


def parse(out):
    d = {}
    for line in out.splitlines():
        name, idx, h = line.split()
        assert int(idx) == len(d.setdefault(name, []))
        d[name].append(h)
    return d


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "regex_compile_digest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def have(tmp_path_factory, golden):
    exe = str(tmp_path_factory.mktemp("regex_digest") / "regex_compile_san")
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tools", "regex_compile_san.cpp")], check=True)
    d = parse(subprocess.run([exe, "--digest", "--blocks", str(BLOCKS)], check=True, capture_output=True, text=True).stdout)
    if d["classes"] != golden["classes"]:
        # the classes are libc's own (regcomp / regexec): another libc moves every struct digest, and says nothing about the compilers
        pytest.skip("this machine's libc gives other byte classes (%s) than the one the digests were recorded with (%s): the recording "
                    "does not apply here" % (d["classes"][0], golden["classes"][0]))
    return d


def test_the_named_tables(have, golden):
    assert have["named"] == golden["named"]


@pytest.mark.parametrize("corpus", ["bytes", "pieces"])
def test_the_first_blocks_of_a_random_corpus(have, golden, corpus):
    assert len(have[corpus]) == BLOCKS
    for k, (h, want) in enumerate(zip(have[corpus], golden[corpus])):
        assert h == want, "block %d of the random corpus '%s' (draws %d..%d)" % (k, corpus, 1000 * k, 1000 * k + 999)


@pytest.mark.parametrize("row", NEW_ROWS)
def test_the_named_tables_through_the_loops_and_the_groups_compiler(have, golden, row):
    assert len(golden[row + ".named"]) == 1 and have[row + ".named"] == golden[row + ".named"]


@pytest.mark.parametrize("corpus", ["bytes", "pieces", "quants"])
@pytest.mark.parametrize("row", NEW_ROWS)
def test_the_first_blocks_of_a_random_corpus_through_the_loops_and_the_groups_compiler(have, golden, row, corpus):
    name = row + "." + corpus
    assert len(have[name]) == BLOCKS and len(golden[name]) >= BLOCKS
    for k, (h, want) in enumerate(zip(have[name], golden[name])):
        assert h == want, "block %d of the random corpus '%s', row '%s' (draws %d..%d)" % (k, corpus, row, 1000 * k, 1000 * k + 999)
