"""lob_run over a directory of recorded days (--md-dir / --tas-dir, data.md_dir / data.tas_dir): the reference's run()
(src/main.cpp:89-239) -- get_file_sample, the train / test split, a training day drawn per book before every episode from the
day library, then the greedy test phase with one row per held-out day, each checked against a greedy one-book engine that
was given that day through lob_load_events and the trained weights."""
import os
import subprocess

import numpy as np
import pytest

from rl_markets_amd import abi, engine
from tests.csv_io import write_reference_csvs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rl_markets_amd", "host", "lob_run")


def day_dirs(tmp_path, lengths, symbol="HSBA.L"):
    md_dir, tas_dir = tmp_path / "md", tmp_path / "tas"
    (md_dir / symbol).mkdir(parents=True)
    (tas_dir / symbol).mkdir(parents=True)
    files = []
    for i, n in enumerate(lengths):
        g = engine.default_gen_params()
        g.n_events = n
        rec = engine.gen_stream_host(g, 5, 2, 300 + i, 1)[0]
        md = str(md_dir / symbol / ("md_202001%02d.csv" % (i + 1)))
        tas = str(tas_dir / symbol / ("tas_202001%02d.csv" % (i + 1)))
        write_reference_csvs(rec, 5, 2, md, tas, date=20200100 + i + 1)
        files.append((md, tas))
    return str(md_dir), str(tas_dir), files


def config(tmp_path, extra):
    src = open(os.path.join(ROOT, "config", "engine.yaml")).read()
    assert "n_episodes: 1000" in src
    path = tmp_path / "days.yaml"
    path.write_text(src.replace("n_episodes: 1000", "n_episodes: 3") + extra)
    return str(path)


def greedy_one_book(md, tas, theta, book):
    p = engine.default_params()          # == config/engine.yaml
    p.algo = abi.ALGO_QLAMBDA
    p.book_id_offset = book
    eng = engine.Engine(p, 1)
    eng.load_events(engine.convert_csv(md, tas))
    eng.set_theta(theta)
    eng.reset()
    for _ in range(100000):
        if eng.counters()[2] == 0:
            break
        eng.eval_step(1)
    eng.clear_inventory()
    d = eng.get_books()[0]
    ntr = d.ask_transactions + d.bid_transactions + d.market_buys + d.market_sells
    out = (d.episode_reward, d.episode_reward / d.total_ticks, d.episode_pnl, ntr)
    eng.close()
    return out


def test_lob_run_days_directory(tmp_path):
    md_dir, tas_dir, files = day_dirs(tmp_path, [700, 520, 860, 610, 750])
    cfg = config(tmp_path, "\nevaluation:\n    n_samples: 2\n")
    theta_file = str(tmp_path / "theta.bin")
    out = subprocess.run([EXE, "-c", cfg, "-a", "q_learn", "-n", "4", "--md-dir", md_dir, "--tas-dir", tas_dir, "--theta", theta_file],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.strip().splitlines()
    assert rows[0] == "episode,episode_id,reward,pnl,n_steps,epsilon"
    train = rows[1:4]
    assert [r.split(",")[0] for r in train] == ["1", "2", "3"]
    for r in train:   # the day book 0 trained on: one of the three training days
        assert r.split(",")[1] in [f[0] for f in files[:3]]
    assert rows[4] == "test,episode,symbol,file,reward,rho,pnl,n_tr,ppt"
    test = [r.split(",") for r in rows[5:]]
    assert len(test) == 2
    theta = np.fromfile(theta_file, dtype=np.float64)
    for i, r in enumerate(test):
        assert r[1] == str(i + 1) and r[2] == "HSBA.L"
        md, tas = files[3 + i]                       # the last two files in glob order
        assert r[3] == md
        rwd, rho, pnl, ntr = greedy_one_book(md, tas, theta, i)
        assert float(r[4]) == pytest.approx(rwd, rel=1e-9, abs=1e-12)
        assert float(r[5]) == pytest.approx(rho, rel=1e-9, abs=1e-12)
        assert float(r[6]) == pytest.approx(pnl, rel=1e-9, abs=1e-12)
        assert int(r[7]) == ntr


def test_lob_run_days_from_config_keys_and_errors(tmp_path):
    md_dir, tas_dir, files = day_dirs(tmp_path, [600, 640, 580])
    cfg = config(tmp_path, "")
    # data.md_dir / data.tas_dir in the config; evaluation.n_samples absent: every day is a test day, none is left to train on
    text = open(cfg).read().replace('symbols: ["HSBA.L"]', 'symbols: ["HSBA.L"]\n    md_dir: "%s"\n    tas_dir: "%s"' % (md_dir, tas_dir))
    open(cfg, "w").write(text)
    out = subprocess.run([EXE, "-c", cfg, "-a", "q_learn", "-n", "2", "-e", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "no training days" in out.stderr
    # evaluation.use_train_sample: the days shuffled with the seed, trained on and tested on
    open(cfg, "a").write("\nevaluation:\n    use_train_sample: true\n    n_samples: 2\n")
    out = subprocess.run([EXE, "-c", cfg, "-a", "q_learn", "-n", "2", "-e", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    test = [r for r in out.stdout.splitlines() if r.startswith("test,") and not r.startswith("test,episode")]
    assert len(test) == 2 and all(r.split(",")[3] in [f[0] for f in files] for r in test)
    # two venues in one engine
    bad = text.replace('symbols: ["HSBA.L"]', 'symbols: ["HSBA.L", "CRDI.MI"]')
    open(cfg, "w").write(bad)
    os.makedirs(os.path.join(md_dir, "CRDI.MI"))
    os.makedirs(os.path.join(tas_dir, "CRDI.MI"))
    out = subprocess.run([EXE, "-c", cfg, "-a", "q_learn", "-n", "2", "-e", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "one venue per engine" in out.stderr
