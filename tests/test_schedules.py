"""Schedules: the reference's own unit vectors (rl_coach/tests/test_schedules.py) and a step-by-step
bit-exact comparison against the values the reference classes themselves produce (tests/golden/schedules.npz,
recorded by tests/golden/make_golden.py)."""
import numpy as np
import pytest

from coach_amd.schedules import ConstantSchedule, ExponentialSchedule, LinearSchedule


def test_constant_and_linear_reference_vectors():
    # rl_coach/tests/test_schedules.py: constant stays; linear reaches its end and stays there
    s = ConstantSchedule(0.3)
    for _ in range(10):
        s.step()
    assert s.current_value == 0.3
    s = LinearSchedule(1, 3, 10)                          # increasing
    vals = []
    for _ in range(15):
        s.step()
        vals.append(float(s.current_value))
    np.testing.assert_allclose(vals[:10], np.linspace(1.2, 3.0, 10))
    assert vals[10:] == [3.0] * 5
    s = LinearSchedule(1.0, 0.1, 4)                       # decreasing
    for _ in range(6):
        s.step()
    assert abs(float(s.current_value) - 0.1) < 1e-15
    s = LinearSchedule(0.1, 0.1, 50000)                   # AdditiveNoiseParameters default: constant
    s.step()
    assert s.current_value == 0.1


def test_exponential_reference_behaviour():
    s = ExponentialSchedule(10, 3, 0.99)
    for _ in range(1000):
        s.step()
    assert s.current_value == 3 and s.current_step == 1000
    with pytest.raises(ValueError):
        ExponentialSchedule(1, 2, 0.9)
    with pytest.raises(ValueError):
        ExponentialSchedule(2, 1, 1.1)


def test_bit_exact_against_reference_classes(golden):
    g = golden("schedules")
    for i, args in enumerate([(1.0, 0.1, 1000), (0.4, 1.0, 333), (1, 0.01, 10000), (1.0, 0, 1000000)]):
        assert list(g["linear_%d_args" % i]) == list(args)
        x, ref = LinearSchedule(*args), g["linear_%d" % i]
        assert len(ref) == 12000
        for t in range(12000):
            x.step()
            assert float(x.current_value) == float(ref[t]), (args, t)
    assert list(g["exponential_args"]) == [1.0, 0.05, 0.995]
    x, ref = ExponentialSchedule(1.0, 0.05, 0.995), g["exponential"]
    assert len(ref) == 2000
    for i in range(2000):
        x.step()
        assert float(x.current_value) == float(ref[i])
