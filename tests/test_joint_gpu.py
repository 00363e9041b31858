"""GPU: joint genotyping (fcsjg_genotype and its _dev twin) equals
the Python restatement of the rules (tests/jg_cases.py) exactly, integer for
integer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fcship
import host_lib as H
import jg_cases as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = J.hand_cases()
NAMES = ("q", "mle", "qual", "kept", "ac", "an", "dp", "pl_off", "src", "gt", "gq", "pl", "n_pl")
SOURCE = open(os.path.join(ROOT, "falcon-genome_amd", "csrc", "joint.hip")).read()
CAPS = {name: int(v) for name, v in re.findall(r"constexpr int (kJg\w+MaxBlocks) = (\d+);", SOURCE)}
BLOCK = int(re.search(r"constexpr int kJgBlock = (\d+);", SOURCE).group(1))
PASSES = (1, 2, 3, 5, 9, 17, 33)   # jg_model_kernel's instantiations: 2 n + 1 <= 64 passes


def same(got, want, what=""):
    for name in NAMES:
        assert np.array_equal(np.asarray(got[name]).reshape(-1), np.asarray(want[name]).reshape(-1)), (what, name)


def device(cohort, pos, n_alt, tabs, minq, gpu, **kw):
    return fcship.jg_genotype(cohort, pos, n_alt, tabs, minq, device=gpu, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_hand_case(gpu, name):
    cohort, pos, n_alt, opts = J.case_arrays(CASES[name])
    tabs, minq = J.tables(1e-3, len(cohort[0]) - 1), J.min_qual(opts.get("conf", 10.0))
    want = J.genotype(cohort, pos, n_alt, tabs, minq)
    assert (want["pl_off"] >= 0).any()
    same(device(cohort, pos, n_alt, tabs, minq, gpu), want, name)


def test_ties_in_mle_and_the_device_s_own_tables(gpu):
    cohort, pos, n_alt, tabs = J.flat_prior_case()
    want = J.genotype(cohort, pos, n_alt, tabs, 0)
    assert list(want["mle"][[0, 6]]) == [1, 0]
    same(device(cohort, pos, n_alt, tabs, 0, gpu), want)
    for a, b in zip(fcship.jg_tables(1e-3, 130), J.tables(1e-3, 130)):
        assert np.array_equal(a, b)


# 2 n + 1 crosses 64 at n = 32 and 128 at n = 64; every instantiation's first and last cohort size
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 130, 159, 160])
def test_cohort_sizes(gpu, n):
    cohort, pos, n_alt = J.random_cohort(200 + n, n, 8 if n > 3 else 40, max_alt=3)
    tabs = J.tables(1e-3, n)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    assert (want["src"] < 0).any() and (want["src"] >= 0).sum() > 4 * n and (want["pl_off"] >= 0).any() and (n_alt > 1).any()
    assert n <= 3 or (want["mle"] > 1).any()
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu), want, n)


@pytest.mark.parametrize("n", [287, 288, 543, 544, 1024])
def test_the_widest_instantiations(gpu, n):
    cohort, pos, n_alt = J.random_cohort(300 + n, n, 2, max_alt=2, no_call=0.1 if n < 1024 else 0.0)
    tabs = J.tables(1e-3, n)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    assert (want["src"] >= 0).sum() > 1.5 * n and (want["mle"] > 3).any()
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu), want, n)


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 257])
def test_site_counts(gpu, sites):
    cohort, pos, n_alt = J.random_cohort(400 + sites, 3, sites, max_alt=3)
    tabs = J.tables(1e-3, 3)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu), want, sites)


def test_every_stride_loop_s_second_trip_and_the_scan_s_second_pass(gpu):
    assert set(CAPS) == {"kJgCellMaxBlocks", "kJgModelMaxBlocks", "kJgSiteMaxBlocks"} and BLOCK == 256
    n = 4
    sites = CAPS["kJgCellMaxBlocks"] * BLOCK // n + 1
    assert sites * n > CAPS["kJgCellMaxBlocks"] * BLOCK                 # a lane per (site, sample): source, genotypes
    assert sites * 6 > CAPS["kJgModelMaxBlocks"] * (BLOCK // 64)        # a wave per (site, ALT): the model
    assert sites > CAPS["kJgSiteMaxBlocks"] * BLOCK and sites > BLOCK   # a lane per site; the scan's passes of a block
    cohort, pos, n_alt = J.random_cohort(77, n, sites, max_alt=2)
    tabs = J.tables(1e-3, n)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    last = np.nonzero(want["pl_off"] >= 0)[0][-1]
    assert last > sites - 50 and want["n_pl"][0] > 3 * n * 1000
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu), want)


def test_positions_near_the_end_of_int32(gpu):
    span = 64
    cohort, pos, n_alt = J.random_cohort(5, 4, 48, max_alt=2, span=span, base=2**31 - 1 - span)
    assert pos.max() >= 2**31 - 6 and cohort[2].max() == 2**31 - 1
    tabs = J.tables(1e-3, 4)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    assert (want["pl_off"][-8:] >= 0).any()
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu), want)


def weak_site():
    """One sample, one site whose ALT is kept (mle = 1) and whose QUAL lies below 10."""
    return ((np.array([0, 1]), np.array([9]), np.array([10]), np.array([1]), np.array([1]), np.array([12]),
             np.array([[36, 0, 60, 40, 70, 90]])), np.array([9]), np.array([1]))


def test_an_empty_site_list_and_a_site_that_fails_the_threshold(gpu):
    cohort, pos, n_alt = J.random_cohort(6, 3, 10)
    tabs = J.tables(1e-3, 3)
    out = device(cohort, pos[:0], n_alt[:0], tabs, J.min_qual(), gpu)
    assert out["n_pl"][0] == 0 and all(len(out[k]) == 0 for k in NAMES if k != "n_pl")
    cohort, pos, n_alt = weak_site()
    tabs = J.tables(1e-3, 1)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    assert want["kept"][0] == 1 and 0 < want["qual"][0] < J.min_qual() and want["n_pl"][0] == 0 and want["pl_off"][0] == -1
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu), want)
    same(device(cohort, pos, n_alt, tabs, int(want["qual"][0]), gpu), J.genotype(cohort, pos, n_alt, tabs, int(want["qual"][0])))
    assert J.genotype(cohort, pos, n_alt, tabs, int(want["qual"][0]))["n_pl"][0] == 3   # the comparison is >=


def test_capacity_exactly_enough_and_one_too_few(gpu):
    cohort, pos, n_alt = J.random_cohort(8, 5, 40, max_alt=3)
    tabs = J.tables(1e-3, 5)
    want = J.genotype(cohort, pos, n_alt, tabs, J.min_qual())
    need = int(want["n_pl"][0])
    assert need > 100
    same(device(cohort, pos, n_alt, tabs, J.min_qual(), gpu, max_pl=need), want)
    with pytest.raises(fcship.FcsError, match=f"have {need} PLs, max_pl is {need - 1}"):
        device(cohort, pos, n_alt, tabs, J.min_qual(), gpu, max_pl=need - 1)
    with pytest.raises(fcship.FcsError, match="positions decrease"):
        bad = [a.copy() for a in cohort]
        bad[1][0], bad[2][0] = cohort[1][1] + 1, cohort[1][1] + 2   # sample 0's first record begins after its second
        device(tuple(bad), pos, n_alt, tabs, J.min_qual(), gpu)


# ------------------------------------------------------------------ the _dev twin
class Twin:
    """fcsjg_genotype_dev on a caller stream with device-resident inputs and outputs."""

    def __init__(self, torch, gpu):
        self.torch, self.gpu = torch, gpu
        self.dev = torch.device(f"cuda:{gpu}")
        self.stream = torch.cuda.Stream(device=self.dev)
        self.keep = []

    def to_dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.dev)

    def queue(self, cohort, pos, n_alt, tabs, minq, max_pl=None, n_records=None):
        torch = self.torch
        n, ns = len(cohort[0]) - 1, len(pos)
        max_pl = ns * n * fcship.FCSJG_GENOTYPES_MAX if max_pl is None else max_pl
        with torch.cuda.stream(self.stream):
            _, arrays = fcship.jg_cohort(*cohort)
            t = [self.to_dev(a) for a in arrays]
            c = fcship.JgCohort(n, 0, len(arrays[1]) if n_records is None else n_records, *(x.data_ptr() for x in t))
            p, a = self.to_dev(np.asarray(pos, np.int32)), self.to_dev(np.asarray(n_alt, np.uint8))
            tt = [self.to_dev(np.asarray(x, np.int32)) for x in tabs]
            st = fcship.JgSites(ns, p.data_ptr(), a.data_ptr())
            m = fcship.JgModel(*(x.data_ptr() for x in tt), minq)
            host = fcship.jg_out_arrays(ns, n, max(max_pl, 1), fill=0x55)
            outs = {k: self.to_dev(v) for k, v in host.items()}
            o = fcship.JgOut(*(outs[name].data_ptr() for name, *_ in fcship.JG_OUT_FIELDS), outs["pl"].data_ptr(), max_pl,
                             outs["n_pl"].data_ptr())
            status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            need = fcship.lib.fcsjg_workspace_bytes(ns, n)
            ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            fcship.check(fcship.lib.fcsjg_genotype_dev(self.gpu, C.addressof(c), C.addressof(st), C.addressof(m), C.addressof(o),
                                                       ws.data_ptr(), need, status.data_ptr(), C.c_void_p(self.stream.cuda_stream)))
        self.keep.append((t, p, a, tt, ws))
        return outs, status

    @staticmethod
    def read(out, n_pl=None):
        outs, status = out
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        got["pl"] = got["pl"][:int(got["n_pl"][0]) if n_pl is None else n_pl]
        return got, int(status.cpu()[0])


def test_dev_twin_on_a_caller_stream(gpu):
    import torch
    twin = Twin(torch, gpu)
    cohort, pos, n_alt = J.random_cohort(11, 6, 70, max_alt=3)
    tabs, minq = J.tables(1e-3, 6), J.min_qual()
    want = J.genotype(cohort, pos, n_alt, tabs, minq)
    need = int(want["n_pl"][0])
    good = twin.queue(cohort, pos, n_alt, tabs, minq)
    enough = twin.queue(cohort, pos, n_alt, tabs, minq, max_pl=need)
    short = twin.queue(cohort, pos, n_alt, tabs, minq, max_pl=need - 1)
    # a PL above the clamp in a source record of a written site: clamped and reported
    site = int(np.nonzero(want["pl_off"] >= 0)[0][0])
    rec = int(want["src"][site * 6:site * 6 + 6].max())
    over = list(cohort)
    over[6] = cohort[6].copy()
    over[6][rec, 0] = fcship.FCSJG_PL_MAX + 7
    clamped = twin.queue(tuple(over), pos, n_alt, tabs, minq)
    # record offsets beyond n_records: clamped and reported
    fewer = twin.queue(cohort, pos, n_alt, tabs, minq, n_records=len(cohort[1]) - 5)
    empty = twin.queue(cohort, pos[:0], n_alt[:0], tabs, minq)
    twin.stream.synchronize()
    got, status = Twin.read(good)
    assert status == 0
    same(got, want)
    same(got, device(cohort, pos, n_alt, tabs, minq, gpu))
    got, status = Twin.read(enough)
    assert status == 0
    same(got, want)
    got, status = Twin.read(short, n_pl=need - 1)
    assert status == fcship.FCSJG_STATUS_PL and got["n_pl"][0] == need and np.array_equal(got["pl"], want["pl"][:-1])
    assert enough[0]["pl"].cpu().numpy()[need:].tolist() == [] and (short[0]["pl"].cpu().numpy()[need - 1:] == 0x55).all()
    got, status = Twin.read(clamped)
    assert status == fcship.FCSJG_STATUS_FIELD
    same(got, J.genotype(tuple(over), pos, n_alt, tabs, minq))
    got, status = Twin.read(fewer)
    cut = list(cohort)
    cut[0] = np.minimum(cohort[0], len(cohort[1]) - 5)
    assert status == fcship.FCSJG_STATUS_FIELD
    same(got, J.genotype(tuple(cut), pos, n_alt, tabs, minq))
    got, status = Twin.read(empty)
    assert status == 0 and got["n_pl"][0] == 0


# ------------------------------------------------------------------ the command
def test_joint_command_gpu_and_host_write_identical_files(gpu, tmp_path):
    contigs = [("ctgA", 4000), ("ctgB", 1500)]
    texts = J.random_gvcfs(41, 6, contigs, sites_per_contig=150)
    os.makedirs(tmp_path / "in")
    with open(tmp_path / "ref.fa", "w") as f:
        for name, ln in contigs:
            f.write(f">{name}\n" + "".join("ACGT"[(k * 7 + k // 5) % 4] for k in range(ln)) + "\n")
    for k, t in enumerate(texts):
        (tmp_path / "in" / f"s{k}.g.vcf").write_text(t)
    logs = {}
    for mode in ("true", "false"):
        p = H.run_cli("joint", "-r", tmp_path / "ref.fa", "-i", tmp_path / "in", "-o", tmp_path / f"{mode}.vcf",
                      env={"FCS_JOINT_GPU": mode, "FCS_GPU_DEVICES": str(gpu), "FCS_JOINT_CHUNK_SITES": "32"}, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        logs[mode] = p.stderr
    assert "(GPU)" in logs["true"] and "(host)" in logs["false"]
    for s in ("", ".gz", ".gz.tbi"):
        assert (tmp_path / f"true.vcf{s}").read_bytes() == (tmp_path / f"false.vcf{s}").read_bytes(), s
    got = (tmp_path / "true.vcf").read_text()
    assert got == J.command_vcf(texts, contigs)
    assert sum(1 for ln in got.splitlines() if not ln.startswith("#")) > 64   # more than two chunks of 32 sites
