"""The mode combinations Rollout.run and Rollout.run_lanes refuse (bgx.rollout._check_modes): all 32
combinations of luck, bearoff, cube, truncate and cube_bearoff, with and without cube0, and the
type checks only run_lanes makes, each with its first message.  The expected messages are
written out below; they were checked once against the methods of the commit before
_check_modes existed.  Everything is refused before the engine or the library is touched:
the methods run on an object without any attribute."""
import itertools

import pytest

import bgx.rollout as R
from bgx.truncate import Truncation

NAMES = ("luck", "bearoff", "cube", "truncate", "cube_bearoff")
OK = "accepted"
NO_CUBE = "cube_bearoff without cube"
CUBE0 = "cube0 without cube"

# modes -> (first message, first message with cube0 given), without the "run: " / "run_lanes: " prefix
EXPECTED = {
    (): (OK, CUBE0),
    ("cube_bearoff",): (NO_CUBE, NO_CUBE),
    ("truncate",): (OK, CUBE0),
    ("truncate", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("cube",): (OK, OK),
    ("cube", "cube_bearoff"): (OK, OK),
    ("cube", "truncate"): ("truncate together with cube is not supported",) * 2,
    ("cube", "truncate", "cube_bearoff"): ("cube_bearoff together with truncate is not supported",) * 2,
    ("bearoff",): (OK, CUBE0),
    ("bearoff", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("bearoff", "truncate"): ("truncate together with bearoff is not supported",) * 2,
    ("bearoff", "truncate", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("bearoff", "cube"): ("cube together with bearoff is not supported",) * 2,
    ("bearoff", "cube", "cube_bearoff"): ("cube_bearoff together with bearoff is not supported",) * 2,
    ("bearoff", "cube", "truncate"): ("truncate together with bearoff is not supported",) * 2,
    ("bearoff", "cube", "truncate", "cube_bearoff"): ("cube_bearoff together with bearoff is not supported",) * 2,
    ("luck",): (OK, CUBE0),
    ("luck", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("luck", "truncate"): (OK, CUBE0),
    ("luck", "truncate", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("luck", "cube"): ("cube together with luck is not supported",) * 2,
    ("luck", "cube", "cube_bearoff"): ("cube_bearoff together with luck is not supported",) * 2,
    ("luck", "cube", "truncate"): ("truncate together with cube is not supported",) * 2,
    ("luck", "cube", "truncate", "cube_bearoff"): ("cube_bearoff together with luck is not supported",) * 2,
    ("luck", "bearoff"): ("bearoff together with luck is not supported",) * 2,
    ("luck", "bearoff", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("luck", "bearoff", "truncate"): ("truncate together with bearoff is not supported",) * 2,
    ("luck", "bearoff", "truncate", "cube_bearoff"): (NO_CUBE, NO_CUBE),
    ("luck", "bearoff", "cube"): ("bearoff together with luck is not supported",) * 2,
    ("luck", "bearoff", "cube", "cube_bearoff"): ("cube_bearoff together with luck is not supported",) * 2,
    ("luck", "bearoff", "cube", "truncate"): ("truncate together with bearoff is not supported",) * 2,
    ("luck", "bearoff", "cube", "truncate", "cube_bearoff"): ("cube_bearoff together with luck is not supported",) * 2,
}

# what only run_lanes can tell, each at its place in the order: (the arguments given, none of
# them of its mode's type; the first message)
WRONG_TYPES = [
    (("truncate",), "truncate must be a truncate.Truncation"),
    (("truncate", "luck"), "truncate must be a truncate.Truncation"),
    (("truncate", "bearoff"), "truncate together with bearoff is not supported"),
    (("truncate", "cube"), "truncate together with cube is not supported"),
    (("truncate", "cube0"), "truncate must be a truncate.Truncation"),
    (("cube", "cube_bearoff"), "cube_bearoff must be a bearoff.CubefulBearoffDB"),
    (("cube", "cube_bearoff", "luck"), "cube_bearoff together with luck is not supported"),
    (("cube_bearoff",), NO_CUBE),
    (("cube", "cube_bearoff", "truncate"), "cube_bearoff together with truncate is not supported"),
    (("cube0",), CUBE0),
    (("cube0", "luck", "bearoff"), "bearoff together with luck is not supported"),
]


class Cubeful:
    kind = "cubeful"


def well_typed():
    return dict(luck=object(), bearoff=object(), cube=object(), truncate=Truncation(lambda eng, tsel: None, 8),
                cube_bearoff=Cubeful())


def first_message(fn, *args, **kw):
    """The ValueError's text; any other end (the dummy object has no engine) means accepted."""
    try:
        fn(*args, **kw)
    except ValueError as e:
        return str(e)
    except Exception:
        pass
    return OK


def prefixed(where, msg):
    return msg if msg == OK else f"{where}: {msg}"


def test_the_table_has_every_combination():
    assert sorted(EXPECTED) == sorted(tuple(n for n, b in zip(NAMES, bits) if b)
                                      for bits in itertools.product((0, 1), repeat=5))


@pytest.mark.parametrize("modes", sorted(EXPECTED))
def test_first_refusal(modes):
    kw = {n: well_typed()[n] for n in modes}
    ro = object.__new__(R.Rollout)
    plain, with_cube0 = EXPECTED[modes]
    assert first_message(R.Rollout.run, ro, None, None, 36, **kw) == prefixed("run", plain)
    assert first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, **kw) == prefixed("run_lanes", plain)
    assert first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, cube0=object(), **kw) \
        == prefixed("run_lanes", with_cube0)
    for where, cube0, msg in (("run", None, plain), ("run_lanes", None, plain), ("run_lanes", object(), with_cube0)):
        got = first_message(R._check_modes, where, cube0=cube0, types=where == "run_lanes", **kw)
        assert got == prefixed(where, msg), (where, cube0 is not None)


@pytest.mark.parametrize("names,msg", WRONG_TYPES)
def test_type_checks_keep_their_place(names, msg):
    kw = {n: 8 if n == "truncate" else object() for n in names}
    ro = object.__new__(R.Rollout)
    assert first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, **kw) == f"run_lanes: {msg}"
    assert first_message(R._check_modes, "run_lanes", types=True, **kw) == f"run_lanes: {msg}"
