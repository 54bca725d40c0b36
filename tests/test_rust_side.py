"""The Rust side of the binding (rust/): what can be checked without rustc.  SURVEY.md section 7 step 9 / north_star
"new holo-spf-hip crate": the crate, the two glue modules and the call-site patches are FILES; here: sys.rs is the
header, the wrapper and the glue only use names that exist."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
RUST = os.path.join(ROOT, "rust")


def _hdr():
    import gen_rust_sys
    return gen_rust_sys.parse(open(gen_rust_sys.HEADER).read())


def test_sys_rs_is_generated_from_the_header_and_current():
    import gen_rust_sys
    assert open(gen_rust_sys.OUT).read() == gen_rust_sys.generate(), "rust/holo-spf-hip/src/sys.rs is stale: python tools/gen_rust_sys.py"


def test_sys_rs_declares_every_function_of_the_header_with_the_same_arity():
    consts, structs, opaques, funcs = _hdr()
    text = open(os.path.join(RUST, "holo-spf-hip", "src", "sys.rs")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "holo_spf_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hspf_[a-z0-9_]+)\s*\(", src))
    declared -= set(re.findall(r"static inline [^;{(]*?\b(hspf_[a-z0-9_]+)\s*\(", src))     # the header's own decode helpers: nothing to bind
    bound = dict((m.group(1), m.group(2)) for m in re.finditer(r"pub fn (hspf_[a-z0-9_]+)\(([^)]*)\)", text))
    assert set(bound) == declared
    for ret, name, params in funcs:
        n = len([p for p in bound[name].split(",") if p.strip()])
        assert n == len(params), name
    assert len(funcs) == len(declared)


def test_repr_c_structs_have_the_header_field_order():
    consts, structs, opaques, funcs = _hdr()
    text = open(os.path.join(RUST, "holo-spf-hip", "src", "sys.rs")).read()
    for name, fields in structs:
        m = re.search(r"#\[repr\(C\)\]\n#\[derive\(Clone, Copy\)\]\npub struct %s \{(.*?)\n\}" % name, text, flags=re.S)
        assert m, name
        got = re.findall(r"pub ([a-z_0-9]+):", m.group(1))
        assert got == [f[1] for f in fields], name
    for name in opaques:
        assert f"pub struct {name} {{ _private: [u8; 0] }}" in text
    for name, val, unsigned in consts:
        assert re.search(r"pub const %s: (u32|i32|usize) = %s;" % (name, re.escape(val)), text), name


@pytest.mark.parametrize("rel", ["holo-spf-hip/src/lib.rs", "holo-isis/src/spf/hip.rs", "holo-ospf/src/spf/hip.rs"])
def test_wrapper_and_glue_only_use_sys_names_that_exist(rel):
    sys_text = open(os.path.join(RUST, "holo-spf-hip", "src", "sys.rs")).read()
    have = set(re.findall(r"pub (?:fn|const|struct) ([A-Za-z_0-9]+)", sys_text))
    text = open(os.path.join(RUST, rel)).read()
    used = set(re.findall(r"\bsys::([A-Za-z_0-9]+)", text))
    assert used and used <= have, sorted(used - have)
    # balanced delimiters: the cheapest "does it parse" there is without a compiler
    code = re.sub(r"//[^\n]*", "", text)
    code = re.sub(r'"(?:\\.|[^"\\])*"', '""', code)
    code = re.sub(r"'(?:\\.|[^'\\])'", "' '", code)
    for a, b in ("()", "[]", "{}"):
        assert code.count(a) == code.count(b), (rel, a, code.count(a), code.count(b))


def test_glue_uses_only_wrapper_items_that_exist():
    lib = open(os.path.join(RUST, "holo-spf-hip", "src", "lib.rs")).read()
    pub = set(re.findall(r"pub (?:fn|struct|mod) ([A-Za-z_0-9]+)", lib))
    for rel in ("holo-isis/src/spf/hip.rs", "holo-ospf/src/spf/hip.rs"):
        text = open(os.path.join(RUST, rel)).read()
        imported = re.search(r"use holo_spf_hip::\{([^}]*)\}", text).group(1)
        for name in [x.strip() for x in imported.split(",")]:
            assert name in pub or name == "sys", (rel, name)
        for meth in ("recommend_cpu", "get_or_patch", "slot_table", "run", "from_env"):
            assert meth in pub
        for meth in re.findall(r"\beng\.([a-z_]+)\(", text) + re.findall(r"\bgraph\.([a-z_]+)\(", text) + re.findall(r"\bcache\.([a-z_]+)\(", text):
            assert meth in pub, (rel, meth)


def test_every_function_of_the_header_has_a_safe_wrapper_or_is_on_the_inspection_list():
    """33 of the 62 ABI functions (every hspf_multi_*, hspf_rib_fold_device) had no Rust wrapper.  Now every
    function of include/holo_spf_hip.h is called by the wrapper crate or the glue — or is one of the inspection / plumbing
    functions below, which a holo build has no use for."""
    consts, structs, opaques, funcs = _hdr()
    text = "".join(open(os.path.join(RUST, rel)).read() for rel in ("holo-spf-hip/src/lib.rs", "holo-isis/src/spf/hip.rs", "holo-ospf/src/spf/hip.rs"))
    used = set(re.findall(r"\bsys::(hspf_[a-z0-9_]+)", text))
    unbound = sorted(name for _, name, _ in funcs if name not in used)
    assert unbound == ["hspf_get_stream", "hspf_graph_n_edges", "hspf_graph_n_edges_kept", "hspf_graph_n_vertices", "hspf_set_stream"], unbound


def _calls(text: str, callee: str) -> list:
    """Argument counts of every call `callee(...)` in Rust source `text` (line comments dropped; a match must not be
    the tail of a longer name; a callee ".name" is a method call)."""
    code = re.sub(r"//[^\n]*", "", text)
    out = []
    head = "" if callee.startswith(".") else r"(?<![A-Za-z0-9_])"
    for m in re.finditer(head + r"%s\(" % re.escape(callee), code):
        depth, i, args, cur = 1, m.end(), [], ""
        while depth:
            c = code[i]
            if c in "([{":
                depth += 1
            elif c in ")]}":
                depth -= 1
            if depth == 1 and c == ",":
                args.append(cur); cur = ""
            elif depth:
                cur += c
            i += 1
        args.append(cur)
        out.append(len([a for a in args if a.strip()]))
    return out


def test_glue_calls_reference_items_that_exist_with_the_reference_arity():
    """The parent-module items the glue relies on: still there, still taking what the glue passes.  The holo side is
    recorded in tests/golden/rust_reference_items.json (names and parameter counts; tools/make_rust_reference_items.py
    re-records it from a holo tree); every call site of the glue is checked against it."""
    import json
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "rust_reference_items.json")))
    fns = ref["functions"]
    for fn, nargs in (("vertex_edges", 6), ("zeroth_lsp", 3), ("resolve_nexthop", 8), ("vertex_networks", 11),
                      ("route_install", 6), ("route_uninstall", 3), ("Route::new", 3), ("Route::distance", 1)):
        assert len(fns[fn]["params"]) == nargs, fn
    glue = open(os.path.join(RUST, "holo-isis", "src", "spf", "hip.rs")).read()
    # every call of a recorded function passes what the recorded signature takes
    for fn in ("vertex_edges", "zeroth_lsp", "resolve_nexthop", "vertex_networks", "route_install", "route_uninstall", "Route::new"):
        got = _calls(glue, fn)
        assert got and all(k == len(fns[fn]["params"]) for k in got), (fn, got)
    got = _calls(glue, ".distance")
    assert got and all(k == len(fns["Route::distance"]["params"]) for k in got), got
    assert glue.count("resolve_nexthop(&mut nexthop, level, mt_id, &parent, &link, &mut used_adjs, interfaces, adjacencies)") == 1
    assert "vertex_edges(vid, mt_id, metric_mode, metric_type, lsdb, lsp_entries)" in glue
    # round 5: the routes / wire step from device tables (hip::update_rib) and the MANET ancestor sets
    assert glue.count("vertex_networks(") == 1 and "Route::new(&vertex, network, level)" in glue
    assert "ibus::tx::route_install(&instance.tx.ibus, &prefix, &route, old_sr_label, distance, interfaces)" in glue
    assert "ibus::tx::route_uninstall(&instance.tx.ibus, &prefix, &route)" in glue
    # the struct the glue builds names every recorded field; the flags it tests exist
    lits = re.findall(r"\bNexthop \{([^{}]*)\}", glue)
    assert lits
    for lit in lits:
        names = [re.split(r"[:\s]", f.strip())[0] for f in lit.split(",") if f.strip()]
        assert sorted(names) == sorted(ref["structs"]["Nexthop"]["fields"]), names
    used_flags = set(re.findall(r"RouteFlags::([A-Z_0-9]+)", glue))
    assert {"INSTALLED", "CONNECTED"} <= used_flags <= set(ref["flags"]["RouteFlags"]["names"]), used_flags
    for name in ("rib_mut", "is_l2_attached_to_backbone"):
        assert name in ref["items"]["holo-isis/src/instance.rs"] and f".{name}(" in glue, name
    # the MANET patch redirects every recorded is_on_path query of flooding/manet.rs
    patch = open(os.path.join(RUST, "patches", "holo-isis.patch")).read()
    removed = [ln for ln in patch.splitlines() if ln.startswith("-") and not ln.startswith("---") and "is_on_path(" in ln]
    assert ref["is_on_path_queries"]["count"] == 3 and len(removed) == ref["is_on_path_queries"]["count"], removed
    g2 = open(os.path.join(RUST, "holo-ospf", "src", "spf", "hip.rs")).read()
    assert "V::calc_nexthops(" in g2 and "V::vertex_lsa_links(" in g2 and "V::vertex_lsa_find(" in g2
    for name in ("vertex_lsa_find", "vertex_lsa_links", "calc_nexthops", "RouteRtr::new", "is_vlink_endpoint", "spf_run_count"):
        assert name in ref["items"]["holo-ospf/src/spf.rs"] and name in g2, name
