"""The device layer's translation units, as the sources state them (nexus_amd/csrc/device): shared kernel text lives in headers, every
unit is in the stale-library check, and every unit with kernel text says so before it includes anything.  Reads sources only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "nexus_amd", "csrc", "device")
KERNEL_HEADERS = ("nx_wavefront.h", "nx_traverse.h")


def sources(pattern):
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(DEVICE, pattern)))}


def includes(text):
    return re.findall(r'^[ \t]*#[ \t]*include[ \t]*["<]([^">]+)[">]', text, re.M)


def test_no_unit_is_included_by_another():
    files = {**sources("*.hip"), **sources("*.h")}
    assert len(files) > 30
    offenders = [(name, inc) for name, text in files.items() for inc in includes(text) if inc.endswith(".hip")]
    assert offenders == [], "shared text belongs in a header (the Makefile's $(HDRS) rebuilds its includers): %s" % offenders


def test_every_unit_is_in_the_layout_stamp_table():
    units = sources("*.hip")
    api = units.pop("nxhip_api.hip")
    table = api[api.index("static int check_layouts()"):api.index("for (const auto& u : units)")]
    named = re.findall(r'\{"([^"]+)",\s*layout_stamp_\w+\(\)\}', table)
    assert len(named) == len(set(named))
    assert sorted(named) == sorted(units), "nxhip_create compares the stamps of exactly the other units (a unit left out escapes the stale-library check)"


def test_units_with_kernel_text_say_so_before_their_first_include():
    units = sources("*.hip")
    headers = sources("*.h")
    kernel_units = [name for name, text in units.items() if set(includes(text)) & set(KERNEL_HEADERS)]
    assert {"nx_wavefront.hip", "nx_wavefront_detail.hip", "nx_wavefront_metal.hip", "nx_wavefront_solid.hip", "nx_medium.hip", "nx_hook_kernels.hip",
            "nx_trace.hip"} <= set(kernel_units)
    for name in kernel_units:
        text = units[name]
        define = re.search(r"^[ \t]*#[ \t]*define[ \t]+NX_KERNEL_TU\b", text, re.M)
        first = re.search(r"^[ \t]*#[ \t]*include\b", text, re.M)
        assert define and define.start() < first.start(), "%s: NX_KERNEL_TU decides whether device pointers are address_space(1) (nx_device.h)" % name
    for name in KERNEL_HEADERS:  # (a header that defined it would hand it to its includers silently)
        assert "define NX_KERNEL_TU" not in headers[name]
