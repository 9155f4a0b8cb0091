"""GPU: the four decode kernels on the packet matrix of tests/packet_matrix.py, with the kernel ASSERTED.

Every section -- lengths, slots, copies, all_pairs, window_fill, limits -- is one launch per LDS-model kernel, forced
through kernel_streams.forced: the full layout sees every stream, the compact and the branchy kernel those that announce
pb <= 2 (everything but the two pb 4 properties of `lengths`).  Every stream is compared with the oracle on bytes, status
and consumed input, every valid one with the crafter's own bytes too, and the three kernels' results with each other by
digest.  The section `hbm` (lengths, copies and window_fill at lc + lp > 8) meets xlz_decode_kernel_hbm_model alone.
Sections 3 and 6 also go through xlz_decode_batch, unsliced and in five slices.  The LZMA2 form of window_fill reads
behind a dictionary reset: the launch flags those streams and the exact re-decode settles them, in every kernel."""
import pytest

import kernel_streams as ks
import lzma_amd
import packet_matrix as pm
import test_gpu_kernels as tk

pytestmark = pytest.mark.gpu

SECTIONS = {
    "lengths": lambda: pm.lengths(),
    "slots": lambda: pm.slots(),
    "copies": lambda: pm.copies() + pm.copies(dict_size=4096),
    "all_pairs": lambda: pm.all_pairs() + pm.last_packets(),
    "window_fill": lambda: pm.window_fill(),
    "limits": lambda: pm.limit_tails() + pm.limits(),
}


def _narrow(cases):
    """the streams a compact-layout launch can hold"""
    return [c for c in cases if ks.announces_pb_up_to_2(c.job[0])]


def _against_crafter(cases, got, what):
    bad = [c.name for c, g in zip(cases, got) if c.crafted is not None and g != (c.crafted, 0, len(c.job[0].data))]
    assert bad == [], "%s: %d valid streams differ from the crafter's bytes, first %s" % (what, len(bad), bad[:10])


def _named(cases, jobs, got, what):
    """_against_oracle with the streams' names in the message"""
    bad = tk.ps.mismatches(jobs, got)
    assert bad == [], "%s: %d of %d streams differ from the oracle, first %s" % (
        what, len(bad), len(jobs), [(cases[i].name, got[i][1:], len(got[i][0]), jobs[i][1]()[1:], len(jobs[i][1]()[0])) for i in bad[:8]])


_CELLS = {}   # (section, kernel) -> digests of the results on the section's streams of pb <= 2


def _cell(ctx, monkeypatch, section, kernel):
    if (section, kernel) in _CELLS:
        return _CELLS[(section, kernel)]
    cases = SECTIONS[section]()
    narrow = _narrow(cases)
    if kernel != "full":
        cases = narrow
    ks.forced(monkeypatch, kernel)
    jobs = pm.jobs(cases)
    streams = [j[0] for j in jobs]
    name, (workgroups, _) = ks.kernel_of(ctx, streams)
    assert name == ks.KERNEL_NAMES[kernel] and workgroups > 0, (section, kernel, name, workgroups)
    got, _ = tk._decode(ctx, streams, "batch")
    assert len(got) == len(jobs)
    what = "%s, %s kernel" % (section, kernel)
    _named(cases, jobs, got, what)
    _against_crafter(cases, got, what)
    by_name = dict(zip((c.name for c in cases), tk._digest(got)))
    _CELLS[(section, kernel)] = [by_name[c.name] for c in narrow]
    return _CELLS[(section, kernel)]


@pytest.mark.parametrize("kernel", tk.KERNELS)
@pytest.mark.parametrize("section", list(SECTIONS))
def test_every_kernel_decodes_every_section(ctx, monkeypatch, section, kernel):
    """one launch per section and kernel: the kernel's name first, then every stream against the oracle and the crafter"""
    cases = SECTIONS[section]()
    assert len({c.name for c in cases}) == len(cases)
    if section == "lengths":
        assert len(_narrow(cases)) == 15 and len(cases) == 25      # pb 4: the full layout alone
    else:
        assert len(_narrow(cases)) == len(cases)
    _cell(ctx, monkeypatch, section, kernel)


@pytest.mark.parametrize("section", list(SECTIONS))
def test_the_three_kernels_agree_on_every_section(ctx, monkeypatch, section):
    """the results do not depend on the kernel: equal digests on the streams all three have seen"""
    cells = {k: _cell(ctx, monkeypatch, section, k) for k in tk.KERNELS}
    assert len(cells["full"]) == len(_narrow(SECTIONS[section]())) > 0
    for k in ("compact", "branchy"):
        assert cells[k] == cells["full"], (section, k)


def test_the_hbm_kernel_decodes_its_sections(ctx, monkeypatch):
    """lengths at (8,1,0) and (5,4,2), copies over both dictionaries and window_fill at (8,1,2): no unit has its model in
    LDS, every packet goes through the checked C++ path of xlz_decode_kernel_hbm_model"""
    ks.unforced(monkeypatch)
    cases = pm.hbm()
    jobs = pm.jobs(cases)
    streams = [j[0] for j in jobs]
    name, (workgroups, _) = ks.kernel_of(ctx, streams)
    assert (name, workgroups) == (ks.KERNEL_NAMES["hbm"], 0), (name, workgroups)
    got, _ = tk._decode(ctx, streams, "batch")
    _named(cases, jobs, got, "hbm")
    _against_crafter(cases, got, "hbm")


def _call(ctx, streams, form):
    """xlz_decode_batch unsliced, or in five shares of the output (64 KiB is less than a fifth of every call here)"""
    if form == "call":
        ctx.set_slicing(0, 0, 1)
    else:
        ctx.set_slicing(1, 1 << 16, 5)
    try:
        return lzma_amd.decode_batch(ctx, streams), ctx.last_call_stats()
    finally:
        ctx.set_slicing(0, 0, 0)


@pytest.mark.parametrize("form", tk.FORMS[1:])
@pytest.mark.parametrize("section", ["copies", "limits"])
def test_the_public_call_decodes_copies_and_limits(ctx, monkeypatch, section, form):
    """sections 3 and 6 through xlz_decode_batch, unsliced and in five slices, with the kernel the library picks.  A call is
    sliced only while its units are one wave round: the 13 695 streams of `limits` go tail by tail, 2739 per call."""
    ks.unforced(monkeypatch)
    cases = SECTIONS[section]()
    groups = [cases] if section == "copies" else [[c for c in cases if c.name.startswith(("limits: %s," % t, "limits: %s behind" % t,
                                                                                          "limits: tail %s" % t))] for t in pm.TAILS]
    assert sum(len(g) for g in groups) == len(cases)
    for k, group in enumerate(groups):
        jobs = pm.jobs(group)
        assert sum(j[0].out_cap for j in jobs) >= 5 << 16
        got, stats = _call(ctx, [j[0] for j in jobs], form)
        few = {key: stats[key] for key in ("slices", "sub_batches", "units", "wave_slots")}
        assert stats["slices"] >= 5 if form == "sliced" else stats["slices"] <= 1, (k, few)
        _named(group, jobs, got, "%s, %s, call %d" % (section, form, k))
        _against_crafter(group, got, "%s, %s, call %d" % (section, form, k))
