"""The one optimisation loop behind train_model, train_pairs and train_sweep (train._optimise), driven with stub engine, feed and writer
objects that append to one event list.  The expected lists below are written out by hand from the three loops the driver replaced (each
entry point's own ``for epoch`` body with ``_final_images`` / ``_ema_images`` / ``_best_images``), not produced by running it."""
import pytest

from splice_amd.train import _optimise


class Engine:
    """Records generate / step / book / window_closes / all_stopped.  ``stop_at``: the step index that closes the window at which every
    slot has stopped.  Images are numbered in the order they are generated (``g0``, ``g1``, ...)."""

    def __init__(self, ev, slots, stop_at=None, ema=False, best=False):
        self.ev, self.slots, self.stop_at = ev, slots, stop_at
        self.ema = "ema" if ema else None
        self.best = "best" if best else None
        self.best_ema = "best_ema" if best and ema else None
        self.step_idx, self.lr, self.images = -1, 0.002, 0

    def generate(self, img, pair=0, track_running_stats=False, ema=False, best=False):
        assert img == f"A{pair}" and not track_running_stats
        self.ev.append(("generate", pair, ema, best))
        self.images += 1
        return [f"g{self.images - 1}"]

    def step(self, a, b, entire):
        self.step_idx += 1
        assert (a, b, entire) == (f"a{self.step_idx}", f"b{self.step_idx}", None)
        self.ev.append(("step", self.step_idx))

    def book_logged_forward(self):
        self.ev.append(("book",))

    def window_closes(self, step_idx):
        self.ev.append(("window_closes", step_idx))
        return step_idx == self.stop_at

    def all_stopped(self):
        self.ev.append(("all_stopped",))
        return True

    def losses(self):
        one = {"loss": 0.5 + self.step_idx}
        return one if self.slots == 1 else [dict(one) for _ in range(self.slots)]


class Writer:
    def __init__(self, ev, slot):
        self.ev, self.slot = ev, slot

    def submit(self, image, force=True, name="output.png"):
        self.ev.append(("submit", self.slot, name, force, image))

    def close(self):
        self.ev.append(("close", self.slot))


def _run(slots, n_epochs, progress=False, callback=True, **engine_kw):
    ev = []
    eng = Engine(ev, slots, **engine_kw)
    feed = iter(range(10 ** 6))

    def next_inputs():
        t = next(feed)
        ev.append(("inputs", t))
        return f"a{t}", f"b{t}", None
    _optimise(dict(n_epochs=n_epochs, log_images_freq=2), eng, next_inputs, [f"A{p}" for p in range(slots)], [Writer(ev, p) for p in range(slots)],
              (lambda p, image: ev.append(("callback", p, image))) if callback else None, progress, single=slots == 1)
    return ev


def _quiet_step(t):
    return [("inputs", t), ("step", t), ("window_closes", t)]


def test_one_slot_five_epochs():
    # train_model: the image of epochs 2 and 4 is generated before the step and written behind its bookkeeping; 4 + 2 > 5 forces the last
    assert _run(1, 5) == _quiet_step(0) + [
        ("inputs", 1), ("generate", 0, False, False), ("step", 1), ("book",), ("submit", 0, "output.png", False, "g0"), ("callback", 0, "g0"),
        ("window_closes", 1)] + _quiet_step(2) + [
        ("inputs", 3), ("generate", 0, False, False), ("step", 3), ("book",), ("submit", 0, "output.png", True, "g1"), ("callback", 0, "g1"),
        ("window_closes", 3)] + _quiet_step(4) + [("close", 0)]


def test_three_slots_five_epochs():
    # train_pairs / train_sweep: every slot's image before the step; behind it one booking, then per slot the writer and the callback
    def logged(t, first, force):
        g = [f"g{first + p}" for p in range(3)]
        return [("inputs", t), ("generate", 0, False, False), ("generate", 1, False, False), ("generate", 2, False, False), ("step", t), ("book",),
                ("submit", 0, "output.png", force, g[0]), ("callback", 0, g[0]), ("submit", 1, "output.png", force, g[1]), ("callback", 1, g[1]),
                ("submit", 2, "output.png", force, g[2]), ("callback", 2, g[2]), ("window_closes", t)]
    assert _run(3, 5) == _quiet_step(0) + logged(1, 0, False) + _quiet_step(2) + logged(3, 3, True) + _quiet_step(4) + [("close", 0), ("close", 1), ("close", 2)]


def test_one_slot_stops_at_step_two():
    assert _run(1, 5, stop_at=2) == _quiet_step(0) + [
        ("inputs", 1), ("generate", 0, False, False), ("step", 1), ("book",), ("submit", 0, "output.png", False, "g0"), ("callback", 0, "g0"),
        ("window_closes", 1),
        ("inputs", 2), ("step", 2), ("window_closes", 2), ("all_stopped",),
        ("generate", 0, False, False), ("submit", 0, "output.png", True, "g1"), ("callback", 0, "g1"),   # the final image, always written
        ("close", 0)]


def test_three_slots_stop_at_step_two():
    assert _run(3, 5, stop_at=2) == _quiet_step(0) + [
        ("inputs", 1), ("generate", 0, False, False), ("generate", 1, False, False), ("generate", 2, False, False), ("step", 1), ("book",),
        ("submit", 0, "output.png", False, "g0"), ("callback", 0, "g0"), ("submit", 1, "output.png", False, "g1"), ("callback", 1, "g1"),
        ("submit", 2, "output.png", False, "g2"), ("callback", 2, "g2"), ("window_closes", 1),
        ("inputs", 2), ("step", 2), ("window_closes", 2), ("all_stopped",),
        ("generate", 0, False, False), ("submit", 0, "output.png", True, "g3"), ("callback", 0, "g3"),   # _final_images: slot by slot
        ("generate", 1, False, False), ("submit", 1, "output.png", True, "g4"), ("callback", 1, "g4"),
        ("generate", 2, False, False), ("submit", 2, "output.png", True, "g5"), ("callback", 2, "g5"),
        ("close", 0), ("close", 1), ("close", 2)]


def test_no_callback():
    assert _run(1, 2, callback=False) == _quiet_step(0) + [
        ("inputs", 1), ("generate", 0, False, False), ("step", 1), ("book",), ("submit", 0, "output.png", True, "g0"), ("window_closes", 1), ("close", 0)]


@pytest.mark.parametrize("n_epochs,stop_at", [(1, None), (5, 0)])
def test_ema_and_best_images_follow_the_loop_one_slot(n_epochs, stop_at):
    # output_ema.png, output_best.png, output_best_ema.png, in that order, no callback -- also behind an early stop
    final = [("all_stopped",), ("generate", 0, False, False), ("submit", 0, "output.png", True, "g0"), ("callback", 0, "g0")] if stop_at == 0 else []
    n = len(final) // 4
    assert _run(1, n_epochs, stop_at=stop_at, ema=True, best=True) == _quiet_step(0) + final + [
        ("generate", 0, True, False), ("submit", 0, "output_ema.png", True, f"g{n}"),
        ("generate", 0, False, True), ("submit", 0, "output_best.png", True, f"g{n + 1}"),
        ("generate", 0, True, True), ("submit", 0, "output_best_ema.png", True, f"g{n + 2}"),
        ("close", 0)]


def test_ema_and_best_images_follow_the_loop_three_slots():
    # _ema_images over the slots, then _best_images: per slot the best weights and, with an average, that step's average
    assert _run(3, 1, ema=True, best=True) == _quiet_step(0) + [
        ("generate", 0, True, False), ("submit", 0, "output_ema.png", True, "g0"),
        ("generate", 1, True, False), ("submit", 1, "output_ema.png", True, "g1"),
        ("generate", 2, True, False), ("submit", 2, "output_ema.png", True, "g2"),
        ("generate", 0, False, True), ("submit", 0, "output_best.png", True, "g3"), ("generate", 0, True, True), ("submit", 0, "output_best_ema.png", True, "g4"),
        ("generate", 1, False, True), ("submit", 1, "output_best.png", True, "g5"), ("generate", 1, True, True), ("submit", 1, "output_best_ema.png", True, "g6"),
        ("generate", 2, False, True), ("submit", 2, "output_best.png", True, "g7"), ("generate", 2, True, True), ("submit", 2, "output_best_ema.png", True, "g8"),
        ("close", 0), ("close", 1), ("close", 2)]


def test_best_without_an_average_and_an_average_alone():
    assert _run(1, 1, best=True) == _quiet_step(0) + [("generate", 0, False, True), ("submit", 0, "output_best.png", True, "g0"), ("close", 0)]
    assert _run(1, 1, ema=True) == _quiet_step(0) + [("generate", 0, True, False), ("submit", 0, "output_ema.png", True, "g0"), ("close", 0)]


@pytest.mark.parametrize("slots", [1, 3])
def test_no_epochs_no_images(slots):
    # step_idx < 0: neither an average image nor a best image; the writers are closed all the same
    assert _run(slots, 0, ema=True, best=True) == [("close", p) for p in range(slots)]


def test_progress_lines(capsys):
    # train_model prints one loss and announces the stop; the other two print the slots' losses, comma-separated, and do not
    _run(1, 5, progress=True, stop_at=2)
    assert capsys.readouterr().out == "Epoch 1: loss=0.5000 lr=0.002\nEpoch 3: the loss has plateaued, stopping\n"
    _run(3, 5, progress=True, stop_at=2)
    assert capsys.readouterr().out == "Epoch 1: loss=0.5000, 0.5000, 0.5000 lr=0.002\n"
    _run(1, 50, progress=True)
    assert capsys.readouterr().out == "Epoch 1: loss=0.5000 lr=0.002\nEpoch 50: loss=49.5000 lr=0.002\n"
    _run(3, 2, progress=False)
    assert capsys.readouterr().out == ""


def test_the_writers_are_closed_when_a_step_raises():
    ev = []
    eng = Engine(ev, 2)

    def broken():
        raise RuntimeError("feed")
    with pytest.raises(RuntimeError, match="feed"):
        _optimise(dict(n_epochs=3, log_images_freq=2), eng, broken, ["A0", "A1"], [Writer(ev, 0), Writer(ev, 1)], None, False)
    assert ev == [("close", 0), ("close", 1)]
