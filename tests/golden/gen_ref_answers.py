#!/usr/bin/env python3
"""Regenerates tests/golden/ref_answers.json: runs the tests that compare with the compiled reference (oracle/_ref, built
by oracle/Makefile where the reference's sources are present) with KREP_RECORD_REF=1, which makes oracle_lib.RefAnswers
store the reference's answers instead of checking them.  Elsewhere those tests compare with the stored answers."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as ol  # noqa: E402

if not (ol.ref_cli() and all(ol.ref_available(lvl) for lvl in ol._REF_FILES)):
    sys.exit("oracle/_ref is incomplete on this host: build it with `make -C oracle all` where the reference's sources are")
sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                          "tests/test_oracle_vs_ref.py", "tests/test_oracle_cli_only_matching.py"],
                         cwd=ROOT, env=dict(os.environ, KREP_RECORD_REF="1")))
