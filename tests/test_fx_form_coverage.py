"""CPU tier: the case table of tests/fx_forms.py reaches every kernel form an effect can take (groove_fx_kernel_form's strings, read
from the library's own table) and sits on both sides of every switch that picks one.  tests/test_gpu_fx_forms.py plays the table."""
from tests import fx_forms as F


def test_tags_name_the_librarys_forms_one_to_one():
    forms = F.library_forms()
    assert len(forms) == len(set(forms)) == len(F.TAGS)
    assert sorted(F.form_of_tag(t, forms) for t in F.TAGS) == sorted(forms)


def test_the_table_reaches_every_form():
    forms = F.library_forms()
    for c in F.CASES:
        assert len(c.walk) == len(c.expect) and all(1 <= f <= 2048 for f in c.walk), c.name
        assert set(c.expect) <= set(F.TAGS), c.name
    reached = {F.form_of_tag(t, forms) for c in F.CASES for t in c.expect}
    unreachable = {F.form_of_tag(t, forms) for t in F.UNREACHABLE_REASONS if t in F.TAGS}
    assert not reached & unreachable
    assert reached | unreachable == set(forms), sorted(set(forms) - reached - unreachable)
    for what, why in sorted(F.UNREACHABLE_REASONS.items()):
        print(f"  unreachable: {what}: {why}")


def test_every_switch_has_a_case_on_each_side():
    for name, side in F.THRESHOLDS.items():
        seen = {}
        for c in F.CASES:
            for f, form in zip(c.walk, c.expect):
                s = side(c, f, form)
                if s is not None:
                    seen.setdefault(s, f"{c.name} @ {f}")
        assert set(seen) == {"below", "above"}, (name, seen)
        print(f"  {name}: {seen['below']} | {seen['above']}")


def test_a_serial_reverb_block_follows_a_direct_one_with_the_allpass_stream_off_and_on():
    """The direct all-pass form swaps the ring bases on the host after every block, and with the all-pass stream on its kernel runs beside
    the ctx stream: the serial kernel of the next block must find the swapped base and wait for that stream.  The walks hold that pair."""
    for direct in (F.DIR, F.DIR_AP):
        assert any((a, b) == (direct, F.R8) for c in F.CASES for a, b in zip(c.expect, c.expect[1:])), direct
    # ... and the other way round, and the chunked form on either side of the serial one
    for pair in ((F.R8, F.DIR), (F.R8, F.DIR_AP), (F.CHK, F.R8), (F.DIR, F.CHK)):
        assert any((a, b) == pair for c in F.CASES for a, b in zip(c.expect, c.expect[1:])), pair


def test_line_lengths_at_the_default_rate():
    """The mirror of the library's line-length derivation, at the figures its documents quote (44.1 kHz)."""
    assert F.delay_frames(0.004) == 176 and F.delay_frames(0.012) == 529 and F.delay_frames(0.0002) == 9
    assert F.chorus_geometry(0.03, 3) == (1323, 441, 441) and F.chorus_geometry(0.0005, 4) == (22, 5, 7)
    assert min(F.comb_frames()) == 1310 and F.allpass_frames() == [221, 75]
    assert F.delay_frames(0.0) == 1 and F.delay_frames(0.1, 48000.0) == 4800
