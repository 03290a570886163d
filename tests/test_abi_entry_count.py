"""Every C ABI entry point that takes a context counts itself (LCGS_ENTRY, csrc/common.hpp): a pipelined forward frame chains
behind the frame before it only if nothing else was asked of the context in between, and it knows that by this count.  An
entry point that enqueued work on the caller's stream without it would race with a chained frame's head -- so the sources
are read here: each `lcgs_status lcgs_*(lcgs_context* ctx, ...)` definition holds exactly one LCGS_ENTRY(ctx), and every such
function the header exports is among them."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc")


def _definitions():
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "abi_*.cpp")) + glob.glob(os.path.join(CSRC, "host", "*.cpp"))):
        text = open(path).read()
        for m in re.finditer(r'^(?:extern "C" )?lcgs_status (lcgs_\w+)\(lcgs_context\* ctx[^;{]*\n\{\n(.*?)^\}\n', text, re.S | re.M):
            out[m.group(1)] = m.group(2)
    return out


def test_every_context_entry_point_counts_itself_once():
    defs = _definitions()
    assert len(defs) >= 70
    for name, body in defs.items():
        assert body.count("LCGS_ENTRY(ctx);") == 1, name
        # ... in front of the first use of the context (argument checks that name it may come first)
        before = body[:body.index("LCGS_ENTRY(ctx);")]
        uses = [ln for ln in before.split("\n") if re.search(r"ctx->|[(,] ?ctx[,)]", ln.split("//")[0]) and "LCGS_REQUIRE(" not in ln]
        assert not uses, (name, uses)


def test_the_header_exports_no_context_function_without_a_definition_that_counts():
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    exported = set(re.findall(r"LCGS_API lcgs_status (lcgs_\w+)\(lcgs_context\* ctx", header))
    assert len(exported) >= 60
    assert exported - {"lcgs_destroy"} <= set(_definitions()) , sorted(exported - set(_definitions()))
