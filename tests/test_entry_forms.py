"""CPU: every way into the library settles the node table's clear debt, or says that it does not.

sdt_gpu_reset leaves the table's clear as a debt (csrc/sdt_ctx.hpp: clear_lo / clear_hi) that the first launches of the level-1 scatter
pay off; no other code may see a table with debt.  So every function that include/sdt_gpu.h declares with a context parameter must
begin -- before any other use of the context's fields -- with one of the two entry forms of sdt_ctx.hpp: SDT_ENTER (sets the device,
settles the debt) or SDT_ENTER_LAZY (sets the device only: the read pushes that end in launch_count and what belongs to them, and reset).  sdt_gpu_destroy
alone keeps a form of its own: it sets the device without checking, because it frees whatever happens.  A function
that only hands the context on must hand it to one that does; the graph unit, which sees the context through sdti::graph_view only,
enters through that (it settles, and every entry point of that unit returns the view's `rc` first: GRAPH_ENTER).  A handful of accessors read host fields and touch no device: they are listed, and checked for that.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soapdenovo-trans_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "sdt_gpu.h")

# host fields only: no device call, nothing of the table
HOST_ONLY = {"sdt_gpu_key_words", "sdt_gpu_table_slots", "sdt_gpu_stream", "sdt_gpu_set_read_ordinal", "sdt_gpu_table_info",
             "sdt_gpu_shard_ranges", "sdt_gpu_kept_batches", "sdt_gpu_screen_info"}
# the entries that do not settle, and why
LAZY = {
    "sdt_gpu_reset": "replaces the debt",
    "push_reads_enqueue": "ends in launch_count",
    "sdt_gpu_count_reads_device": "ends in launch_count",
    "sdt_gpu_push_wait": "waits for a push's copy: part of the push",
    "sdt_gpu_hint_total_kmers": "a hint before the first push; touches the table through grow_table only, which settles",
}
# frees the table with its debt, and frees even if the device cannot be set: `(void)hipSetDevice(c->device)`, no entry form
DESTROY = "sdt_gpu_destroy"
DESTROY_FORM = "(void)hipSetDevice(c->device);"


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".cuh")):
            out[name] = _strip_comments(open(os.path.join(CSRC, name)).read())
    return out


def _declared():
    """name -> True for every function of the header with a context parameter"""
    text = _strip_comments(open(HEADER).read())
    names = []
    for m in re.finditer(r"\b(sdt_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bsdt_ctx\s*\*\s*\w+", m.group(2)) and not re.search(r"\bsdt_ctx\s*\*\s*\*", m.group(2).split(",")[0]):
            names.append(m.group(1))
    return names


def _definition(sources, name):
    """(file, context parameter's name, body) of the definition of `name`"""
    for fname, text in sources.items():
        for m in re.finditer(r"^[\w:\*\s\"]*?\b%s\s*\(([^;{}]*?)\)\s*\{" % re.escape(name), text, flags=re.M | re.S):
            pm = re.search(r"\bsdt_ctx\s*\*\s*(\w+)", m.group(1))
            if not pm:
                continue
            depth, i = 1, m.end()
            while depth and i < len(text):
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
            return fname, pm.group(1), text[m.end():i]
    return None


def _enters(sources, name, seen=()):
    """None if `name` begins with an entry form (directly or through the first function it hands its context to), else what is wrong"""
    d = _definition(sources, name)
    if d is None:
        return f"{name}: no definition found in csrc/"
    fname, c, body = d
    use = re.search(r"\b%s->" % re.escape(c), body)
    forms = [m for m in (re.search(r"\bSDT_ENTER(_LAZY)?\(%s\)" % re.escape(c), body), re.search(r"\bsdti::graph_view\(\s*(\(sdt_ctx \*\))?%s\)" % re.escape(c), body)) if m]
    entry = min(forms, key=lambda m: m.start()) if forms else None
    if entry is not None and (use is None or entry.start() < use.start()):
        if entry.group(0).startswith("SDT_ENTER_LAZY") and name not in LAZY:
            return f"{name} ({fname}) enters without settling the clear debt and is not one of the listed exceptions"
        if entry.group(0).startswith("SDT_ENTER(") and name in LAZY:
            return f"{name} ({fname}) is listed as an entry that does not settle, but settles"
        return None
    # no form before the first use of a field: the context must go, untouched, to a function that enters
    head = body[:use.start()] if use else body
    for m in re.finditer(r"\b(\w+)\s*\(\s*(?:\(sdt_ctx \*\))?%s\s*[,)]" % re.escape(c), head):
        callee = m.group(1)
        if callee in ("fail", "sizeof") or callee in seen or callee == name:
            continue
        if _definition(sources, callee) is None:
            continue
        return _enters(sources, callee, seen + (name,))
    return f"{name} ({fname}): uses {c}-> before SDT_ENTER / SDT_ENTER_LAZY" if use else f"{name} ({fname}): neither an entry form nor a callee that has one"


def test_every_context_function_begins_with_an_entry_form():
    sources = _sources()
    names = _declared()
    assert len(names) > 100, len(names)               # (the header declares some 150 of them: the parse found them)
    wrong = []
    for name in names:
        if name in HOST_ONLY:
            _, c, body = _definition(sources, name)
            if re.search(r"\bhip[A-Z]\w*\s*\(|<<<|Launch|d_ent|d_aux|d_first", body):
                wrong.append(f"{name}: listed as host-only but touches the device")
            continue
        if name == DESTROY:
            _, c, body = _definition(sources, name)
            use = re.search(r"\bc->", body)
            if "SDT_ENTER" in body or "settle_clear" in body or body.find(DESTROY_FORM) != use.start() - len("(void)hipSetDevice("):
                wrong.append(f"{name}: must begin with {DESTROY_FORM} and neither settle nor return early")
            continue
        bad = _enters(sources, name)
        if bad:
            wrong.append(bad)
    assert not wrong, "\n".join(wrong)


def test_the_lazy_entries_are_the_listed_ones():
    text = "".join(_sources().values())
    assert "#define SDT_ENTER_LAZY(c)" in text and "#define SDT_ENTER(c)" in text
    uses = re.findall(r"\bSDT_ENTER_LAZY\((\w+)\)", text)
    # the listed ones -- and the macro's definition and SDT_ENTER's expansion of it
    assert len(uses) == len(LAZY) + 2, uses
    # nobody sets the device of a context by hand any more
    assert not re.search(r"hipSetDevice\(\s*c\s*->\s*device\s*\)", text.replace("#define SDT_ENTER_LAZY(c) HIPCHK(hipSetDevice((c)->device))", "").replace(DESTROY_FORM, "", 1)), \
        "an entry point sets the device without an entry form"


def test_the_debt_is_settled_where_the_table_is_needed():
    """the inner places that the read pushes reach without an entry that settles"""
    src = _sources()
    body = lambda text, head: text[text.index(head):].split("\n}\n", 1)[0]
    gpu, pipe = src["sdt_gpu.hip"], src["sdt_pipeline.hip"]
    for where, head in ((gpu, "int grow_table("), (gpu, "int ensure_room("), (gpu, "static int launch_count("), (pipe, "int sk_count_all("),
                        (pipe, "int sk_scatter_launch(")):
        assert "settle_clear(c)" in body(where, head), head
    # the graph unit: graph_view enters (and keeps what failed in the view), every entry point of the unit returns that first
    assert "SDT_ENTER(c)" in body(gpu, "static int graph_enter(") and "v.rc = graph_enter(c)" in body(gpu, "sdti::GraphView sdti::graph_view(")
    graph = src["sdt_gpu_graph.hip"]
    entries = re.findall(r"^(?:extern \"C\" )?int (sdt_gpu_\w+)\(sdt_ctx \*c\b", graph, flags=re.M)
    assert len(entries) >= 20, entries
    for name in entries:
        b = body(graph, "int %s(sdt_ctx *c" % name)
        m = re.search(r"const GraphView (v0?) = sdti::graph_view\(c\);", b)
        if not m:
            assert not re.search(r"\bhip[A-Z]\w*\s*\(|LAUNCH", b), name        # (a setter of host fields)
            continue
        # behind the view and the checks of the arguments, in front of the first call that touches the device
        enter = b.find("GRAPH_ENTER(%s);" % m.group(1))
        dev = re.search(r"\bhip[A-Z]\w*\s*\(|LAUNCH|<\w+>\(c\b|sdti::\w+\(c\b(?<!graph_view\(c)", b[m.end():])
        assert enter > m.start() and (dev is None or enter < m.end() + dev.start()), name
    # only reset creates debt
    assert len(re.findall(r"clear_hi\s*=\s*c->slots", gpu + pipe)) == 1 and "clear_hi = c->slots" in body(gpu, "int sdt_gpu_reset(")
