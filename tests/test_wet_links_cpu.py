"""CPU tier: what the wet-dry-mix links add above the library, as far as it can be seen without a device — the project loader accepts
`controls` onto `wet-dry-mix` (an LFO's resolves; a signal source's is dropped with a warning and HELD for an orchestrator with
set_wet_links_on_device), the two new orchestrator switches are off by default, and the library's list of effect kernel forms is what it
was (a partly wet reverb in the run reports the existing strings)."""
import os
import subprocess

import pytest

from groove_amd.host_binding import HOST_LIB
from tests import fx_forms as F
from tests.test_project_controllers import LFO, TAP, describe, host, project  # noqa: F401  (host: the fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTROLS = ('{id: "breathe", source: "wobble", target: {id: "verb", param: "wet-dry-mix"}},'
            '{id: "duck-the-tail", source: "tap", target: {id: "verb", param: "wet-dry-mix"}},'
            '{id: "sweep", source: "tap", target: {id: "lp", param: "cutoff"}}')

PROGRAM = r'''
#include "project.hpp"
#include <cstdio>
#include <fstream>
#include <sstream>
using namespace groove_host;
int main(int argc, char** argv) {
  std::ifstream f(argv[argc - 1]);
  std::stringstream text;
  text << f.rdbuf();
  const ProjectDesc p = parse_project(text.str(), "");
  for (const auto& h : p.held_controls) std::printf("held %s %d\n", h.control.id.c_str(), held_control_is_wet(h.control) ? 1 : 0);
  Orchestrator o(0, GROOVE_DEFAULT_SAMPLE_RATE, 120.0);   // (without a device it has no context; the switches are the host's own)
  std::printf("switches %d %d\n", o.wet_links_on_device() ? 1 : 0, o.wet_reverb_run() ? 1 : 0);
  std::printf("kinds %d %d %d\n", fx_control_device_wet(GROOVE_FX_REVERB, GROOVE_CTL_FX_WET) ? 1 : 0, fx_control_device_wet(GROOVE_FX_MIXER, GROOVE_CTL_FX_WET) ? 1 : 0,
              fx_control_device_wet(GROOVE_FX_REVERB, GROOVE_CTL_FX_ATTENUATION) ? 1 : 0);
  return 0;
}
'''


def test_the_loader_accepts_controls_onto_wet_dry_mix(host):  # noqa: F811
    d = describe(host, text=project(LFO + TAP, CONTROLS))
    assert d["warnings"] == 2                                    # the two signal sources onto parameters the host path cannot serve
    assert d["controls"] == [{"id": "breathe", "source": "wobble", "target": "verb", "param": "wet-dry-mix", "route": "per-block"}]


def test_held_controls_and_switch_defaults(host, tmp_path):  # noqa: F811
    """A program of the test's own over the host layer's headers: the signal control onto wet-dry-mix is held for set_wet_links_on_device
    (and the one onto a cutoff for set_filter_links_on_device, as before); a new Orchestrator has both new switches off."""
    host_dir = os.path.dirname(HOST_LIB)
    src, exe, proj = tmp_path / "check.cpp", tmp_path / "check", tmp_path / "p.json5"
    src.write_text(PROGRAM)
    proj.write_text(project(LFO + TAP, CONTROLS))
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I", host_dir, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    "-L", host_dir, "-lgroove_host", "-L", os.path.dirname(host_dir), "-lgroove_hip",
                    f"-Wl,-rpath,{host_dir}", f"-Wl,-rpath,{os.path.dirname(host_dir)}"], check=True)
    out = subprocess.run([str(exe), str(proj)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    assert out == ["held duck-the-tail 1", "held sweep 0", "switches 0 0", "kinds 1 0 0"], out


def test_the_form_names_are_what_they_were():
    """No new FxForm: 17 strings, each named by exactly one tag of tests/fx_forms.py, in the table's order."""
    forms = F.library_forms()
    assert len(forms) == len(F.TAGS) == 17
    assert [F.form_of_tag(t, forms) for t in F.TAGS] == forms
