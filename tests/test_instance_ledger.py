"""The ledger of compiled kernel instances, as the sources state them: every set a unit lists in an Instances<...> is valid under
nx_variants.h's rules, every set the host's feature functions (nxhip_render.hip) can ask for is listed in the unit the host looks it up
in (nx_host.h), and every listed set has a case in tests/instance_matrix_reference.py's tables — a new instance without a case fails
here, on the CPU.  Reads sources only; the rules and the four feature functions are restated in Python from their comments, and the
restatement is held to the static_assert cases of nxhip_render.hip.  No count is written down here: the lists are what they are."""
import itertools
import os
import re

from tests import instance_matrix_reference as M

DEVICE = M.DEVICE
C = M.constants()
NX_MAT = {"NX_MAT_DIFFUSE": 0, "NX_MAT_DIELECTRIC": 1, "NX_MAT_PLASTIC": 2, "NX_MAT_CONDUCTOR": 3, "NX_MAT_METALROUGH": 4}


def _read(name):
    return open(os.path.join(DEVICE, name)).read()


def _units():
    return {name: _read(name) for name in sorted(os.listdir(DEVICE)) if name.endswith(".hip")}


def _value(expr, names):
    """a set as a unit spells it: 0u, or constants joined by |"""
    total = 0
    for term in expr.split("|"):
        term = term.strip()
        if re.fullmatch(r"\d+u?", term):
            total |= int(term.rstrip("u"))
        else:
            assert term in names, "a set spelled with something that is no constant of nx_variants.h: %r" % term
            total |= names[term]
    return total


def _lists():
    """every Instances<...> of the device units: [(unit, name or None, [sets])]"""
    out = []
    for unit, text in _units().items():
        for m in re.finditer(r"(?:using\s+(\w+)\s*=\s*)?Instances<([^<>;{}]*)>", text):
            out.append((unit, m.group(1), [_value(e, C) for e in m.group(2).split(",")]))
    return out


def _families():
    """the lists by what they are lists OF, found from the lookup that uses each:
    {"scan": {unit: sets}, "tail": {unit: sets}, "classic": {unit: (types, sets)}, "medium": sets, "trace": sets, "logic": sets}"""
    named = {(unit, name): sets for unit, name, sets in _lists() if name}
    fam = {"scan": {}, "tail": {}, "classic": {}, "medium": None, "trace": None, "logic": None}
    used = set()
    for unit, text in _units().items():
        def sets_of(name):
            used.add((unit, name))
            return named[(unit, name)]
        for m in re.finditer(r"shade_scan_instance<(\w+)>\(set\)", text):
            fam["scan"][unit] = sets_of(m.group(1))
        for m in re.finditer(r"tail_instance<(\w+)>\(set\)", text):
            fam["tail"][unit] = sets_of(m.group(1))
        for m in re.finditer(r"shade_instance<(\w+),([^>]*)>\(type, set\)", text):
            fam["classic"][unit] = ([NX_MAT[t.strip()] for t in m.group(2).split(",")], sets_of(m.group(1)))
        for m in re.finditer(r"(\w+)::find\(set, \[\]\(auto f\) \{ return \(const void\*\)medium_scatter_kernel<", text):
            fam["medium"] = sets_of(m.group(1))
        for m in re.finditer(r"(\w+)::find\(\w+, \[\]\(auto f\) \{ return \(const void\*\)trace_kernel<", text):
            fam["trace"] = sets_of(m.group(1))
    anonymous = [(unit, sets) for unit, name, sets in _lists() if name is None]
    assert len(anonymous) == 1 and "logic_kernel" in _read(anonymous[0][0]), "an Instances<...> without a name that is not the logic kernel's: %s" % anonymous
    fam["logic"] = anonymous[0][1]
    assert used == set(named), "a list of instances this ledger knows no family for: %s" % sorted(set(named) - used)
    assert fam["medium"] and fam["trace"] and fam["scan"] and fam["tail"] and fam["classic"]
    return fam


# ---- nx_variants.h's rules, restated -----------------------------------------------------------------------------------------------------------

POWER, NO_MAPS, ANALYTIC, DETAIL, METAL, SOLID, TREE, MF_ALL = (C["kMf" + n] for n in ("Power", "NoMaps", "Analytic", "Detail", "Metal", "Solid", "Tree", "All"))
ANY_HIT, COUNTING, ENTRY, IDENTITY, TRANSMIT, ALPHA_TEST, TF_ALL = (C["kTf" + n] for n in ("AnyHit", "Counting", "Entry", "Identity", "Transmit", "AlphaTest", "All"))
SHADE_READS, TAIL_READS, MEDIUM_READS, LOGIC_READS = POWER | ANALYTIC | DETAIL | SOLID, POWER | ANALYTIC | DETAIL | METAL, POWER | ANALYTIC | METAL | TREE, ANALYTIC


def material_set_ok(f):
    """SOLID => METAL => DETAIL => not NO_MAPS; TREE => POWER and not NO_MAPS"""
    if f & ~MF_ALL:
        return False
    if f & SOLID and not f & METAL:
        return False
    if f & METAL and not f & DETAIL:
        return False
    if f & DETAIL and f & NO_MAPS:
        return False
    if f & TREE and (not f & POWER or f & NO_MAPS):
        return False
    return True


def material_closure(f):
    """the smallest valid set over f"""
    if f & SOLID:
        f |= METAL
    if f & METAL:
        f |= DETAIL
    if f & DETAIL:
        f &= ~NO_MAPS
    if f & TREE:
        f = (f | POWER) & ~NO_MAPS
    return f


def shade_set_ok(f, metal_type):
    """the classic pipeline's kernels: the TYPE says what METAL would; no map-free and no TREE form"""
    return not f & ~SHADE_READS and material_set_ok(f | (METAL if metal_type or f & SOLID else 0))


def tail_set_ok(f):
    """no map-free form, no SOLID one, no TREE one"""
    return not f & ~TAIL_READS and material_set_ok(f)


def medium_set_ok(f):
    """the light sample's three features and the fifth type's hit code, no closure: TREE => POWER is all"""
    return not f & ~MEDIUM_READS and (not f & TREE or bool(f & POWER))


def trace_set_ok(f):
    """IDENTITY and ENTRY have no counting form; ENTRY is a closest-hit launch's; TRANSMIT: the general any-hit instance and its counting
    variant; ALPHA_TEST: the general instances and their counting variants"""
    if f & ~TF_ALL:
        return False
    if f & COUNTING and f & (IDENTITY | ENTRY):
        return False
    if f & ENTRY and f & ANY_HIT:
        return False
    if f & TRANSMIT and (not f & ANY_HIT or f & (ENTRY | IDENTITY)):
        return False
    if f & ALPHA_TEST and f & (ENTRY | IDENTITY):
        return False
    return True


# ---- nxhip_render.hip's feature functions, restated from their comments ---------------------------------------------------------------------------

RENDER = _read("nxhip_render.hip")
FLAVOR = {name: int(value) for name, value in re.findall(r"\b(kFlavor[A-Z]\w*) = (\d+)\b", RENDER)}


def _fl(name):
    return FLAVOR["kFlavor" + name]


def material_features(flavor):
    """what the SCAN material launch and the tail kernel are instances of: the flavor's facts, the tree only in POWER mode under SCAN, the
    map-free form only under SCAN, then the closure"""
    f = 0
    if flavor & _fl("LightPower"):
        f |= POWER
    if flavor & _fl("LightTree") and flavor & _fl("LightPower") and flavor & _fl("Scan"):
        f |= TREE
    for bit, feature in (("Analytic", ANALYTIC), ("Detail", DETAIL), ("Metal", METAL), ("Solid", SOLID)):
        if flavor & _fl(bit):
            f |= feature
    if flavor & _fl("NoMaps") and flavor & _fl("Scan"):
        f |= NO_MAPS
    return material_closure(f)


def shade_features(flavor, mat_type):
    """the classic kernel of one type: METAL goes unless the type is the fifth (and the DETAIL it implied with it)"""
    return material_features(flavor if mat_type == NX_MAT["NX_MAT_METALROUGH"] else flavor & ~_fl("Metal")) & SHADE_READS


def tail_features(flavor):
    """no map-free form"""
    return material_features(flavor) & ~NO_MAPS


def medium_features(flavor):
    """the facts it reads, and no closure"""
    return material_features(flavor & (_fl("Scan") | _fl("LightPower") | _fl("LightTree") | _fl("Analytic") | _fl("Metal"))) & MEDIUM_READS


def logic_features(flavor, items):
    """the one-item instance alone has the ANALYTIC form"""
    return material_features(flavor) & LOGIC_READS if items == 1 else 0


def trace_features(flavor, any_hit, primary, counting):
    f = (ANY_HIT if any_hit else 0) | (COUNTING if counting else 0)
    if flavor & _fl("Identity"):
        f |= IDENTITY
    if flavor & _fl("Entry") and primary and not any_hit:
        f |= ENTRY
    if flavor & _fl("Transmit") and any_hit:
        f |= TRANSMIT
    if flavor & _fl("AlphaTest"):
        f |= ALPHA_TEST
    if f & COUNTING:
        f &= ~(IDENTITY | ENTRY)
    if f & ALPHA_TEST:
        f &= ~(IDENTITY | ENTRY)
    if f & TRANSMIT:
        f &= ~IDENTITY
    return f


FEATURE_BITS = ("Scan", "LightPower", "LightTree", "Analytic", "Detail", "Metal", "Solid", "NoMaps", "Identity", "Entry", "Transmit", "AlphaTest")


def _flavors():
    """every combination of the flavor bits a feature function reads (pass_flavor produces fewer: the functions are asked about all)"""
    for on in itertools.product((0, 1), repeat=len(FEATURE_BITS)):
        yield sum(_fl(name) for name, bit in zip(FEATURE_BITS, on) if bit)


def test_the_feature_functions_read_no_other_flavor_bit():
    """the enumeration below covers the functions' whole domain: the kFlavor constants their texts name are FEATURE_BITS"""
    text = RENDER[RENDER.index("constexpr unsigned material_features(int flavor)"):RENDER.index("// (build-time tests of the selection")]
    assert set(re.findall(r"kFlavor(\w+)", text)) == set(FEATURE_BITS)


def test_the_restatement_passes_the_static_assert_cases():
    """every static_assert of nxhip_render.hip that calls a feature function, evaluated with the functions above"""
    block = RENDER[RENDER.index("// (build-time tests of the selection"):RENDER.index("std::vector<std::vector<Launch>> frame_levels")]
    cases = re.findall(r"static_assert\((.*?),\s*\n\s*\"([^\"]*)\"\);", block, re.S)
    assert len(cases) >= 8
    names = dict(C, **FLAVOR, **NX_MAT, material_features=material_features, shade_features=shade_features, tail_features=tail_features, medium_features=medium_features,
                 logic_features=logic_features, trace_features=trace_features, true=True, false=False)
    checked = 0
    for expr, what in cases:
        if "_features(" not in expr:
            continue
        for term in expr.replace("\n", " ").split("&&"):
            py = re.sub(r"\b(\d+)u\b", r"\1", term.strip())
            assert eval(py, {"__builtins__": {}}, names) is True, "%s: %s" % (what, term.strip())  # noqa: S307 (the project's own source text)
            checked += 1
    assert checked >= 25


# ---- (a) every listed set is valid -------------------------------------------------------------------------------------------------------------------

def test_every_listed_set_is_valid_and_listed_once():
    fam = _families()
    for unit, sets in fam["scan"].items():
        assert len(set(sets)) == len(sets) and all(material_set_ok(s) for s in sets), unit
    for unit, sets in fam["tail"].items():
        assert len(set(sets)) == len(sets) and all(tail_set_ok(s) for s in sets), unit
    for unit, (types, sets) in fam["classic"].items():
        assert len(set(sets)) == len(sets), unit
        for t in types:
            assert all(shade_set_ok(s, t == NX_MAT["NX_MAT_METALROUGH"]) for s in sets), (unit, t)
    assert len(set(fam["medium"])) == len(fam["medium"]) and all(medium_set_ok(s) for s in fam["medium"])
    assert len(set(fam["trace"])) == len(fam["trace"]) and all(trace_set_ok(s) for s in fam["trace"])
    assert all(not s & ~LOGIC_READS for s in fam["logic"])
    # no set stands in two units of one family: the host looks a set up in ONE unit (nx_host.h)
    for family in ("scan", "tail"):
        every = [s for sets in fam[family].values() for s in sets]
        assert len(set(every)) == len(every), family


# ---- (b) every set the host can ask for is listed, in the unit the host asks ------------------------------------------------------------------------

def _unit_of(set_, mat_type=None):
    """nx_host.h kernels::shade_scan / tail / shade: the units split the instances by their newest feature"""
    if set_ & SOLID:
        return "nx_wavefront_solid.hip"
    if mat_type is None and set_ & METAL or mat_type == NX_MAT["NX_MAT_METALROUGH"]:
        return "nx_wavefront_metal.hip"
    if set_ & DETAIL:
        return "nx_wavefront_detail.hip"
    return "nx_wavefront.hip"


def test_the_host_header_dispatches_as_restated():
    host = _read("nx_host.h")
    assert "(set & kMfSolid) ? wavefront_solid::shade_scan(set) : (set & kMfMetal) ? wavefront_metal::shade_scan(set) : (set & kMfDetail) ? wavefront_detail::shade_scan(set) : wavefront::shade_scan(set)" in host
    assert "(set & kMfMetal) ? wavefront_metal::tail(set) : (set & kMfDetail) ? wavefront_detail::tail(set) : wavefront::tail(set)" in host
    assert "(set & kMfSolid) ? wavefront_solid::shade(type, set) : type == NX_MAT_METALROUGH ? wavefront_metal::shade(type, set) : (set & kMfDetail) ? wavefront_detail::shade(type, set) : wavefront::shade(type, set)" in host


def _reachable():
    """{family: the sets the feature functions return over every flavor, and the rules allow}"""
    out = {"scan": set(), "tail": set(), "medium": set(), "trace": set(), "classic": set(), "logic": set()}
    for flavor in _flavors():
        if flavor & _fl("Scan"):
            out["scan"].add(material_features(flavor))
            out["tail"].add(tail_features(flavor))
            out["medium"].add(medium_features(flavor))
        else:
            for t in NX_MAT.values():
                out["classic"].add((t, shade_features(flavor, t)))
            out["logic"].add(logic_features(flavor, 1))
        for any_hit, primary, counting in itertools.product((False, True), repeat=3):
            if not (any_hit and primary):  # (the primary launch is a closest-hit one)
                out["trace"].add(trace_features(flavor, any_hit, primary, counting))
    out["scan"] = {s for s in out["scan"] if material_set_ok(s)}
    out["tail"] = {s for s in out["tail"] if tail_set_ok(s)}
    out["medium"] = {s for s in out["medium"] if medium_set_ok(s)}
    out["trace"] = {s for s in out["trace"] if trace_set_ok(s)}
    out["classic"] = {(t, s) for t, s in out["classic"] if shade_set_ok(s, t == NX_MAT["NX_MAT_METALROUGH"])}
    return out


def test_every_set_the_host_can_ask_for_is_listed():
    """nxhip_render.hip: "a set no unit compiled — unreachable while the units' lists cover the feature functions".  This is that sentence."""
    fam, reach = _families(), _reachable()
    assert material_features(0) == 0 and all(material_set_ok(material_features(f)) for f in _flavors()), "material_features ends in the closure: every set it returns is valid"
    for s in sorted(reach["scan"]):
        assert s in fam["scan"].get(_unit_of(s), ()), "the SCAN material launch of set %s (%d): not in %s" % (M.set_name(s), s, _unit_of(s))
    for s in sorted(reach["tail"]):
        assert s in fam["tail"].get(_unit_of(s), ()), "the tail kernel of set %s (%d): not in %s" % (M.set_name(s), s, _unit_of(s))
    for t, s in sorted(reach["classic"]):
        types, sets = fam["classic"].get(_unit_of(s, t), ((), ()))
        assert t in types and s in sets, "the classic material kernel of type %d, set %s (%d): not in %s" % (t, M.set_name(s), s, _unit_of(s, t))
    for s in sorted(reach["medium"]):
        assert s in fam["medium"], "the medium's scatter kernel of set %s (%d)" % (M.set_name(s), s)
    for s in sorted(reach["trace"]):
        assert s in fam["trace"], "trace_kernel of set %s (%d)" % (M.set_name(s, "kTf"), s)
    assert reach["logic"] <= set(fam["logic"])
    # ... and nothing is compiled that no flavor asks for: a listed set nobody can launch is dead code no test can reach
    assert {s for sets in fam["scan"].values() for s in sets} == reach["scan"]
    assert {s for sets in fam["tail"].values() for s in sets} == reach["tail"]
    assert set(fam["medium"]) == reach["medium"] and set(fam["trace"]) == reach["trace"]
    assert {(t, s) for types, sets in fam["classic"].values() for t in types for s in sets} == reach["classic"]


# ---- (c) every listed set has a case -------------------------------------------------------------------------------------------------------------------

def test_every_listed_set_has_a_case():
    fam = _families()
    listed = {"scan": {s for sets in fam["scan"].values() for s in sets}, "tail": {s for sets in fam["tail"].values() for s in sets}, "medium": set(fam["medium"]), "trace": set(fam["trace"]),
              "classic": {(t == NX_MAT["NX_MAT_METALROUGH"], s) for types, sets in fam["classic"].values() for t in types for s in sets}}
    tables = {"scan": M.SCAN_CASES, "tail": M.TAIL_CASES, "medium": M.MEDIUM_CASES, "trace": M.TRACE_CASES, "classic": M.CLASSIC_CASES}
    for family, sets in listed.items():
        missing = sets - set(tables[family])
        assert not missing, "%s: compiled instances without a case in tests/instance_matrix_reference.py: %s" % (family, sorted(missing))
        extra = set(tables[family]) - sets
        assert not extra, "%s: cases for sets no unit lists: %s" % (family, sorted(extra))
    # a case's key is what its description spells: the tables are keyed by set, not by position
    for key, case in M.SCAN_CASES.items():
        assert key == M.mf(*M.FAMILY[case["family"]], *M.SAMPLING[case["sampling"]], *(("Analytic",) if case["analytic"] else ()))
