"""The device report writers' float formatter (csrc/shortest_f64.h: Schubfach shortest digits, the ryu and Rust
Display layouts) run on the host through gg_format_f64, against the oracle's formatters, which sit on Python's
correctly rounded shortest repr: every output byte-equal."""
import random
import struct

import pytest

import guard_amd
from guard_oracle import pv

# layout thresholds, rounding ties, the subnormal / normal / overflow ends, 17-digit results, and the powers of two
# (the lower half of their rounding interval is half as wide: the asymmetric case of every shortest algorithm)
EDGES = [0.0, -0.0, 2.5, 0.1, 0.3, 1e15, 1e16, 123456789012345680.0, 1e21, 1e22, 1e23, 1e-5, 1e-4, 1e-7,
         5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308, 2.0 ** 53, 2.0 ** 53 + 2,
         4.35, 0.30000000000000004, 9007199254740993.0, -2.5, -1e-7, -1.7976931348623157e308]
EDGES += [2.0 ** k for k in range(-1074, 1024, 37)] + [2.0 ** k for k in (-1022, -1021, -1, 1, 52, 54, 63, 64, 1023)]


def _both(x):
    return guard_amd.format_f64(x, 0), guard_amd.format_f64(x, 1)


@pytest.mark.parametrize("x", EDGES, ids=repr)
def test_edges(x):
    assert _both(x) == (pv.ryu_f64(x), pv.rust_display_f64(x))


@pytest.mark.parametrize("x,ryu,display", [
    (-0.0, "-0.0", "-0"), (1e16, "1e16", "10000000000000000"), (1e21, "1e21", "1000000000000000000000"),
    (1e-5, "0.00001", "0.00001"), (1e-7, "1e-7", "0.0000001"), (123456789012345680.0, "1.2345678901234568e17", "123456789012345680"),
])
def test_layouts_as_written_out(x, ryu, display):
    assert _both(x) == (ryu, display)


def test_random_bit_patterns_and_short_decimals():
    rng = random.Random(20240611)
    xs = []
    for _ in range(40000):   # uniform over sign, finite exponents and significands
        bits = (rng.getrandbits(1) << 63) | (rng.randrange(0, 2047) << 52) | rng.getrandbits(52)
        xs.append(struct.unpack("<d", struct.pack("<Q", bits))[0])
    for _ in range(4000):
        xs.append(float("%d.%d" % (rng.randrange(0, 10 ** rng.randrange(1, 18)), rng.randrange(0, 10 ** rng.randrange(1, 6)))))
        xs.append(float("%de%d" % (rng.randrange(1, 1000), rng.randrange(-330, 306))))
    bad = [x for x in xs if _both(x) != (pv.ryu_f64(x), pv.rust_display_f64(x))]
    assert not bad, [(x.hex(), _both(x)) for x in bad[:5]]


def test_non_finite_is_refused():
    assert guard_amd.format_f64(float("inf")) is None and guard_amd.format_f64(float("nan"), 1) is None
