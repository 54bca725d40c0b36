#!/usr/bin/env python3
"""tools/make_rust_reference_items.py — record what the Rust glue (rust/) relies on in the holo tree it is written
against: names and parameter counts of the functions it calls, the fields of the struct it builds, the flag constants and
methods it uses, and the number of Spt::is_on_path queries the MANET patch redirects.  Only names and numbers are
written (tests/golden/rust_reference_items.json); tests/test_rust_side.py checks the glue's call sites against them.

usage: python tools/make_rust_reference_items.py <holo source tree>
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rust_reference_items.json")


def _params(text: str, pattern: str, drop_self: bool = False) -> list:
    m = re.search(pattern, text, flags=re.S)
    assert m, pattern
    names = [a.split(":")[0].strip() for a in m.group(1).split(",") if a.strip()]
    if drop_self:
        names = [a for a in names if a not in ("self", "&self", "&mut self")]
    return names


def _fn(text: str, name: str, generic: bool = True, vis: str = "", drop_self: bool = False) -> list:
    gen = r"(?:<[^>]*>)?" if generic else ""
    return _params(text, r"%sfn %s%s\(\s*(.*?)\)\s*(?:->|\{)" % (vis, re.escape(name), gen), drop_self)


def extract(ref: str) -> dict:
    def src(rel):
        return open(os.path.join(ref, rel)).read()
    isis, route, tx = src("holo-isis/src/spf.rs"), src("holo-isis/src/route.rs"), src("holo-isis/src/ibus/tx.rs")
    inst, manet, ospf = src("holo-isis/src/instance.rs"), src("holo-isis/src/flooding/manet.rs"), src("holo-ospf/src/spf.rs")
    funcs = {}
    for name in ("vertex_edges", "zeroth_lsp", "resolve_nexthop", "vertex_networks"):
        funcs[name] = {"file": "holo-isis/src/spf.rs", "params": _fn(isis, name)}
    for name in ("route_install", "route_uninstall"):
        funcs[name] = {"file": "holo-isis/src/ibus/tx.rs", "params": _fn(tx, name, generic=False, vis=r"pub\(crate\) ")}
    funcs["Route::new"] = {"file": "holo-isis/src/route.rs", "params": _fn(route, "new", generic=False, vis=r"pub\(crate\) ")}
    funcs["Route::distance"] = {"file": "holo-isis/src/route.rs",
                                "params": _fn(route, "distance", generic=False, vis=r"pub\(crate\) const ", drop_self=True)}
    m = re.search(r"pub struct Nexthop \{(.*?)\n\}", route, flags=re.S)
    assert m
    fields = re.findall(r"^\s*pub ([a-z_0-9]+):", m.group(1), flags=re.M)
    flags = re.findall(r"const ([A-Z_0-9]+) = ", re.search(r"struct RouteFlags: \w+ \{(.*?)\}", route, flags=re.S).group(1))
    items = {"holo-isis/src/instance.rs": [n for n in ("rib_mut", "is_l2_attached_to_backbone") if f"pub(crate) fn {n}(" in inst],
             "holo-ospf/src/spf.rs": [n for n, probe in (("vertex_lsa_find", "fn vertex_lsa_find("), ("vertex_lsa_links", "fn vertex_lsa_links<'a>("),
                                                         ("calc_nexthops", "fn calc_nexthops("), ("RouteRtr::new", "RouteRtr::new("),
                                                         ("is_vlink_endpoint", "is_vlink_endpoint()"), ("spf_run_count", "spf_run_count += 1"))
                                      if probe in ospf]}
    queries = manet.count("spt_hopcount.is_on_path(") + manet.count(".spt_hopcount\n                .is_on_path(")
    return {"tree": "holo " + re.search(r'^version = "([^"]+)"', src("Cargo.toml"), flags=re.M).group(1),
            "functions": funcs,
            "structs": {"Nexthop": {"file": "holo-isis/src/route.rs", "fields": fields}},
            "flags": {"RouteFlags": {"file": "holo-isis/src/route.rs", "names": flags}},
            "items": items,
            "is_on_path_queries": {"file": "holo-isis/src/flooding/manet.rs", "count": queries}}


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "holo-isis")):
        sys.exit(__doc__)
    with open(OUT, "w") as f:
        json.dump(extract(sys.argv[1]), f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)


if __name__ == "__main__":
    main()
