"""[EXT] codec preambles and prompt stems, the lifecycle they share: HeldTable of csrc/sched_logic.h, driven alone.  Who holds an object (its
creator, the voices and the engine-level setting it is set on, the requests that took it), in which order a setter swaps, what a build that
ends after its release does, and every message the table produces.  These rules decide whether a device snapshot or a KV store is freed
under a request that still restores from it.  The table is built with plain g++ and the host sanitizers, like the other rule drivers.  No
GPU is used."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDING, READY, FAILED = 0, 1, -1
NOUNS = ("preamble", "stem")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("held_logic") / "held_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "held_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


class Session:
    """One table: commands are collected with their expected answers and run in one go; show() parses the table's contents."""

    def __init__(self, driver, noun):
        self.driver, self.cmds, self.want = driver, ["new %s" % noun], ["ok"]

    def do(self, cmd, want):
        self.cmds.append(cmd)
        self.want.append(want)
        return self

    def show(self, engine, voices, entries):
        """entries: {id: (creator, holders, state, n, payload)}"""
        body = "".join(" %d=%d/%d/%d/%d/%d" % ((i,) + tuple(e)) for i, e in sorted(entries.items()))
        return self.do("show", "engine %d voices %d %d %d live %d :%s" % ((engine,) + tuple(voices) + (len(entries), body)))

    def run(self):
        got = self.driver("\n".join(self.cmds) + "\n")
        for cmd, want, have in zip(self.cmds, self.want, got):
            assert have == want, (cmd, self.cmds)
        assert len(got) == len(self.want)


NONE = (-1, -1, -1)


@pytest.mark.parametrize("noun", NOUNS)
@pytest.mark.parametrize("ok", (1, 0))
def test_release_while_building_recycles_when_the_build_ends(driver, noun, ok):
    s = Session(driver, noun).do("add 6 77", "0").show(-1, NONE, {0: (1, 0, BUILDING, 6, 77)})
    s.do("release 0", "kept").show(-1, NONE, {0: (0, 0, BUILDING, 6, 77)})   # its build still writes what it owns
    s.do("finish 0 %d" % ok, "recycled 77").show(-1, NONE, {})
    s.do("finish 0 1", "kept")                                               # a second end finds nothing
    s.run()


@pytest.mark.parametrize("noun", NOUNS)
def test_finish_then_release_without_holders_recycles_at_the_release(driver, noun):
    for ok, state in ((1, READY), (0, FAILED)):
        s = Session(driver, noun).do("add 4 5", "0").do("finish 0 %d" % ok, "kept").show(-1, NONE, {0: (1, 0, state, 4, 5)})
        s.do("release 0", "recycled 5").show(-1, NONE, {}).run()


@pytest.mark.parametrize("noun", NOUNS)
def test_a_voice_keeps_a_released_object_until_it_is_set_elsewhere(driver, noun):
    for unset in ("voice 1 -1", "voice 1 1"):
        s = Session(driver, noun).do("add 3 10", "0").do("add 3 11", "1").do("finish 0 1", "kept").do("finish 1 1", "kept")
        s.do("voice 1 0", "kept").do("release 0", "kept").show(-1, (-1, 0, -1), {0: (0, 1, READY, 3, 10), 1: (1, 0, READY, 3, 11)})
        s.do("voice 0 -1", "kept")                                           # another voice that was set to nothing
        s.do(unset, "recycled 10")
        other = 1 if unset.endswith(" 1") else -1
        s.show(-1, (-1, other, -1), {1: (1, 1 if other == 1 else 0, READY, 3, 11)}).run()
    # the same with the engine-level setting and a request as the last holders
    s = Session(driver, noun).do("add 3 10", "0").do("finish 0 1", "kept").do("engine 0", "kept").do("hold 0", "ok").do("release 0", "kept")
    s.show(0, NONE, {0: (0, 2, READY, 3, 10)}).do("engine -1", "kept").show(-1, NONE, {0: (0, 1, READY, 3, 10)})
    s.do("unhold 0", "recycled 10").show(-1, NONE, {}).run()


@pytest.mark.parametrize("noun", NOUNS)
def test_setting_the_same_id_twice_never_recycles_it(driver, noun):
    Session(driver, noun).do("add 2 9", "0").do("finish 0 1", "kept").do("release 0", "recycled 9").run()   # nobody held it: the control
    s = Session(driver, noun).do("add 2 9", "0").do("finish 0 1", "kept").do("voice 2 0", "kept").do("engine 0", "kept").do("release 0", "kept")
    s.show(0, (-1, -1, 0), {0: (0, 2, READY, 2, 9)})
    for _ in range(2):   # the new hold is taken before the old one is dropped; a drop first would recycle it here
        s.do("voice 2 0", "kept").show(0, (-1, -1, 0), {0: (0, 2, READY, 2, 9)})
        s.do("engine 0", "kept").show(0, (-1, -1, 0), {0: (0, 2, READY, 2, 9)})
    s.do("engine -1", "kept").do("voice 2 0", "kept").show(-1, (-1, -1, 0), {0: (0, 1, READY, 2, 9)})
    s.do("voice 2 -1", "recycled 9").show(-1, NONE, {}).run()


@pytest.mark.parametrize("noun", NOUNS)
def test_a_setter_refuses_what_is_not_ready_and_changes_nothing(driver, noun):
    s = Session(driver, noun).do("add 1 20", "0").do("add 1 21", "1").do("add 1 22", "2").do("finish 0 1", "kept").do("finish 2 0", "kept")
    s.do("voice 0 0", "kept").do("engine 0", "kept")
    table = {0: (1, 2, READY, 1, 20), 1: (1, 0, BUILDING, 1, 21), 2: (1, 0, FAILED, 1, 22)}
    s.show(0, (0, -1, -1), table)
    refusals = ((9, "unknown %s id" % noun), (1, "the %s is still building: wait for it (q3tts_%s_wait)" % (noun, noun)), (2, "the %s failed to build" % noun))
    for bad, why in refusals:
        s.do("refusal %d" % bad, why)
        for setter in ("voice 0 %d", "voice 1 %d", "engine %d"):
            s.do(setter % bad, "throw " + why).show(0, (0, -1, -1), table)
    s.do("refusal 0", "ok")
    for setter in ("voice 0 -7", "voice 1 -7", "engine -7", "engine -2"):
        s.do(setter, "throw %s id must be -1 (none) or a %s's id" % (noun, noun)).show(0, (0, -1, -1), table)
    s.run()


@pytest.mark.parametrize("noun", NOUNS)
def test_a_double_release_throws_and_ids_are_never_reused(driver, noun):
    s = Session(driver, noun).do("add 1 30", "0").do("finish 0 1", "kept").do("hold 0", "ok").do("release 0", "kept")
    s.do("release 0", "throw the %s has already been released" % noun).show(-1, NONE, {0: (0, 1, READY, 1, 30)})
    s.do("unhold 0", "recycled 30").do("release 0", "throw unknown %s id" % noun).do("at 0", "throw unknown %s id" % noun).do("find 0", "0")
    s.do("hold 0", "throw unknown %s id" % noun)
    s.do("add 1 31", "1").do("release 1", "kept").do("finish 1 0", "recycled 31").do("add 1 32", "2").do("at 2", "1").do("find 2", "1")
    s.show(-1, NONE, {2: (1, 0, BUILDING, 1, 32)}).run()


@pytest.mark.parametrize("noun", NOUNS)
def test_unhold_of_an_unknown_id_is_a_no_op(driver, noun):
    s = Session(driver, noun).do("unhold 0", "kept").do("unhold -1", "kept").do("add 1 40", "0").do("unhold 5", "kept")
    s.show(-1, NONE, {0: (1, 0, BUILDING, 1, 40)}).run()


@pytest.mark.parametrize("noun", NOUNS)
@pytest.mark.parametrize("seed", (1, 20260, 977))
def test_random_walk_against_a_model_that_recounts_every_holder(driver, noun, seed):
    out = driver("walk %s %d 4000\n" % (noun, seed))[0]
    assert out.startswith("ok "), out            # a failure names its seed and step
    assert int(out.split()[1]) > 100, out        # the walk did recycle: it is not a walk over an ever-growing table


def test_messages_are_the_ten_exact_strings(driver):
    want = {
        "preamble": ("unknown preamble id", "the preamble has already been released",
                     "the preamble is still building: wait for it (q3tts_preamble_wait)", "the preamble failed to build",
                     "preamble id must be -1 (none) or a preamble's id"),
        "stem": ("unknown stem id", "the stem has already been released", "the stem is still building: wait for it (q3tts_stem_wait)",
                 "the stem failed to build", "stem id must be -1 (none) or a stem's id"),
    }
    for noun in NOUNS:
        # id 0 stays building, id 1 fails, id 2 is released once; each message comes from the operation that produces it
        got = driver("new %s\nadd 1 1\nadd 1 2\nadd 1 3\nfinish 1 0\nfinish 2 1\nhold 2\nrelease 2\n"
                     "at 7\nrelease 2\nengine 0\nengine 1\nengine -3\n" % noun)[-5:]
        assert tuple(got) == tuple("throw " + m for m in want[noun]), noun
