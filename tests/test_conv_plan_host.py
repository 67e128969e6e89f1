"""The kernel rule of the convolutions (cerberus_amd/csrc/conv_plan.h) without a GPU: tests/tools/conv_plan_main.cpp (its own main, includes only that
header) compiled with the system C++ compiler, asked at the rule's boundaries; the expected answers are written out here."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

ALGOS = (0, 1, 5, 6, 7)
# (cin, cout) of the network's 3x3 stride-1 layers: the four residual stages, the decoder levels (cerb_net_finalize)
PAIRS = ((64, 64), (128, 128), (256, 256), (512, 512), (256, 128), (128, 64))
MAPS = ((4, 4), (8, 8), (14, 14), (16, 16), (28, 28), (32, 32), (56, 56), (64, 64), (64, 80), (112, 112), (128, 128), (256, 256), (448, 448))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "tools", "conv_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(queries):
        """queries: dicts of the rule's inputs (defaults: a Winograd-packed 3x3 stride-1 64 -> 64 layer, algo 6, NHWC, inference) -> [(kernel, family)]"""
        keys = ("algo", "ks", "stride", "cin", "cout", "ho", "wo", "wino", "mode", "planar", "train", "resid", "packed", "site")
        base = dict(algo=6, ks=3, stride=1, cin=64, cout=64, ho=64, wo=64, wino=1, mode=0, planar=0, train=0, resid=0, packed=0, site=-1)
        text = "".join(" ".join(str(int(dict(base, **q)[k])) for k in keys) + "\n" for q in queries)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        out = [tuple(line.split(" ", 1)) for line in r.stdout.splitlines()]
        assert len(out) == len(queries)
        return out

    return run


def kernels(ask, queries):
    return [k for k, _ in ask(queries)]


def test_default_algorithm_by_map_size(ask):
    """algo 6: F(2x2) below 16 x 16; conv_wino4b from 16 x 16 to 64 x 64 where the contraction is whole 64-channel blocks, else conv_wino4; conv_wino4 above"""
    q = [dict(ho=8, wo=8), dict(ho=15, wo=17), dict(ho=16, wo=16), dict(ho=64, wo=64), dict(ho=16, wo=16, cin=32), dict(ho=64, wo=64, cin=96),
         dict(ho=64, wo=80), dict(ho=128, wo=128), dict(ho=8, wo=8, cin=32)]
    assert kernels(ask, q) == ["wino2", "wino2", "wino4b", "wino4b", "wino4", "wino4", "wino4", "wino4", "wino2"]


def test_fixed_algorithms(ask):
    for ho, wo in MAPS:
        for cin in (32, 64, 96, 128, 512):
            q = [dict(algo=a, ho=ho, wo=wo, cin=cin) for a in (0, 1, 5, 7)]  # 0 direct, 1 F(2x2), 5 never conv_wino4b, 7 always where the contraction allows
            assert kernels(ask, q) == ["igemm", "wino2", "wino4", "wino4b" if cin % 64 == 0 else "wino4"], (ho, wo, cin)
    # algo 1: F(2x2) for every Winograd-packed layer; a layer that is not packed is direct under every algorithm
    assert kernels(ask, [dict(algo=a, wino=0) for a in ALGOS]) == ["igemm"] * 5


def test_stride_2_and_1x1_are_direct_under_every_algorithm(ask):
    q = [dict(algo=a, ks=ks, stride=s, wino=w, ho=ho, wo=ho) for a in ALGOS for ks, s in ((3, 2), (1, 1), (1, 2)) for w in (0, 1) for ho in (8, 32, 128)]
    assert set(kernels(ask, q)) == {"igemm"}
    # the decoder entry of the direct path (skip + upsampled map summed on the load) exists in the direct kernel only
    assert set(kernels(ask, [dict(algo=a, mode=1) for a in ALGOS])) == {"igemm"}


def test_planar_only_where_an_f4_kernel_would_run_on_folded_weights(ask):
    ok = [dict(planar=1, site=3, ho=16, wo=16), dict(planar=1, site=3, ho=256, wo=256), dict(planar=1, site=0, ho=32, wo=32, cin=256, cout=128),
          dict(planar=1, site=4, algo=5), dict(planar=1, site=4, algo=7), dict(planar=1, site=4, cin=48)]
    assert kernels(ask, ok) == ["wino4p"] * len(ok)
    bad = [dict(planar=1, ho=8, wo=8), dict(planar=1, algo=0), dict(planar=1, algo=1), dict(planar=1, train=1), dict(planar=1, mode=1), dict(planar=1, wino=0),
           dict(planar=1, ks=1, wino=0), dict(planar=1, stride=2, wino=0, train=1), dict(planar=1, stride=2, wino=0, mode=1)]
    assert kernels(ask, bad) == ["none"] * len(bad)
    # a planar stage's stride-2 entry: the direct kernel's planar epilogue, whatever the algorithm
    entry = [dict(planar=1, stride=2, wino=0, ks=ks, algo=a) for ks in (3, 1) for a in ALGOS]
    assert kernels(ask, entry) == ["igemm_planar"] * len(entry)


def test_data_gradient_takes_the_forward_kernel_of_the_swapped_layer(ask):
    """the data gradient of a layer (Cin, Cout) is asked as the stride-1 convolution Cout -> Cin, Winograd-packed where make_conv packs wino_dgrad
    (Cin % 64 == 0, Cout % 32 == 0): on every (cin, cout) of the network's 3x3 stride-1 layers the forward layer cin -> cout and the data gradient of
    the layer cout -> cin run the same kernel on the same map"""
    for cin, cout in PAIRS:
        for algo in ALGOS:
            fwd = [dict(algo=algo, cin=cin, cout=cout, ho=h, wo=w, wino=cin % 32 == 0, train=1) for h, w in MAPS]
            layer_cin, layer_cout = cout, cin  # the layer whose data gradient this is
            dgr = [dict(algo=algo, cin=layer_cout, cout=layer_cin, ho=h, wo=w, wino=layer_cin % 64 == 0 and layer_cout % 32 == 0, train=1) for h, w in MAPS]
            a, b = ask(fwd), ask(dgr)
            assert a == b, (cin, cout, algo)
            if algo == 6:
                assert [k for k, _ in a] == ["wino2"] * 3 + ["wino4b"] * 5 + ["wino4"] * 5, (cin, cout)


def test_family_names(ask):
    q = [dict(ho=8, wo=8), dict(ho=8, wo=8, resid=1), dict(ho=128, wo=128), dict(ho=128, wo=128, resid=1), dict(), dict(resid=1), dict(ho=56, wo=56, packed=1),
         dict(ho=56, wo=56, packed=1, resid=1), dict(planar=1, site=0), dict(planar=1, site=1), dict(planar=1, site=2), dict(planar=1, site=3),
         dict(planar=1, site=4), dict(planar=1, site=4, resid=1), dict(planar=1, site=4, stride=2, wino=0, ho=16, wo=16), dict(planar=1, site=4, stride=2, ks=1, wino=0),
         dict(algo=0, mode=1), dict(ks=1, wino=0, ho=16, wo=16), dict(ks=3, stride=2, wino=0)]
    assert ask(q) == [("wino2", "conv_wino<f2x2,8x16>"), ("wino2", "conv_wino<f2x2,8x16,res>"), ("wino4", "conv_wino4<f4x4,16x16x2>"),
                      ("wino4", "conv_wino4<f4x4,16x16x2,res>"), ("wino4b", "conv_wino4b<f4x4,16x16>"), ("wino4b", "conv_wino4b<f4x4,16x16,res>"),
                      ("wino4b", "conv_wino4b<f4x4,16t>"), ("wino4b", "conv_wino4b<f4x4,16t,res>"), ("wino4p", "conv_wino4_planar<f4x4,16x16x2,eighth-res>"),
                      ("wino4p", "conv_wino4_planar<f4x4,16x16x2,quarter-res>"), ("wino4p", "conv_wino4p<f4x4,16x16x2,planar,half-res>"),
                      ("wino4p", "conv_wino4p<f4x4,16x16x2,planar>"), ("wino4p", "conv_wino4_enc<f4x4,16x16x2>"), ("wino4p", "conv_wino4_enc<f4x4,16x16x2,res>"),
                      ("igemm_planar", "conv_igemm_planar<ks3,s2,16x16>"), ("igemm_planar", "conv_igemm_planar<ks1,s2,8x32>"),
                      ("igemm", "conv_igemm<ks3,s1,mode1,8x32>"), ("igemm", "conv_igemm<ks1,s1,mode0,16x16>"), ("igemm", "conv_igemm<ks3,s2,mode0,8x32>")]
