"""Every arena tag of the step driver is requested at one site.

An Arena (sx_tree.hpp) finds a buffer by its tag, and a larger request under the same tag frees and reallocates it.
A tag requested from two places with sizes that drift apart, or misspelt at one of them, is an out-of-bounds access
or a silently emptied buffer, not a compile error.  So sx_sim*.cpp and sx_bdt.cpp request each tag once, store the
pointer in a typed struct on the sim (SkinBuffers, DomBuffers, GravBuffers, sx_sim.hpp), and read it from there.
The "dt.*" tags of DevTree::reserve and the "nb.*" tags of NbLists::reserve live in sx_tree.hpp, outside this rule.
"""
import collections
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(__file__), "..", "sph-exa_amd", "csrc")
TAG = re.compile(r'\b(?:get|pinned)\s*<[^<>;()]*>\s*\(\s*(?:std::string\(\s*)?"([^"]+)"')


def test_each_arena_tag_is_requested_once():
    files = sorted(glob.glob(os.path.join(CSRC, "sx_sim*.cpp"))) + [os.path.join(CSRC, "sx_bdt.cpp")]
    assert len(files) >= 5, files
    sites = collections.defaultdict(list)
    for path in files:
        with open(path) as f:
            text = f.read()
        for m in TAG.finditer(text):
            line = text.count("\n", 0, m.start()) + 1
            sites[m.group(1)].append("%s:%d" % (os.path.basename(path), line))
    assert len(sites) > 100, "the pattern no longer finds the arena requests"
    twice = {tag: where for tag, where in sites.items() if len(where) > 1}
    assert not twice, "arena tags requested at more than one site: %r" % twice
