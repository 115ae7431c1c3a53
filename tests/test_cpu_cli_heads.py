"""The contradicting combinations of the gallery, dense-head and depth-head options in cli.main are parser errors: the argparse exit status, a message
on stderr that names the options, no traceback -- before any file is opened or any device touched."""
import pytest

M = ["-m", "none.gguf"]
DENSE = ["--dense-head", "h.npz", "--dense-out", "m.pgm"]
DEPTH = ["--depth-head", "d.npz", "--depth-out", "d.npy"]
BUILD = ["--gallery-build", "dir", "--gallery-out", "g.npz"]

CASES = [
    (DENSE + ["--dir", "d"], "--dense-head labels the single image of -i"),
    (DENSE + ["--gallery", "g.npz"], "--dense-head labels the single image of -i"),
    (DENSE + BUILD, "--dense-head labels the single image of -i"),
    (DEPTH + DENSE, "not together with --dense-head"),
    (DEPTH + ["--dir", "d"], "--depth-head measures the single image of -i"),
    (DEPTH + ["--gallery", "g.npz"], "--depth-head measures the single image of -i"),
    (DEPTH + BUILD, "--depth-head measures the single image of -i"),
    (["--gallery", "g.npz"] + BUILD, "--gallery searches for the single image of -i"),
    (["--gallery", "g.npz", "--dir", "d"], "--gallery searches for the single image of -i"),
    (["--gallery-build", "dir"], "--gallery-build DIR and --gallery-out G.npz go together"),
    (["--gallery-out", "g.npz"], "--gallery-build DIR and --gallery-out G.npz go together"),
    (["--dense-head", "h.npz"], "--dense-head HEAD.npz and --dense-out PATH go together"),
    (["--dense-out", "m.pgm"], "--dense-head HEAD.npz and --dense-out PATH go together"),
    (["--depth-head", "d.npz"], "--depth-head HEAD.npz and --depth-out PATH.npy go together"),
    (["--depth-out", "d.npy"], "--depth-head HEAD.npz and --depth-out PATH.npy go together"),
    (BUILD + ["--img-fit", "28"], "--img-fit takes its shape from the single image of -i, not --gallery-build"),
]


@pytest.mark.parametrize("argv,message", CASES, ids=[" ".join(a for a in c[0] if a.startswith("--")) for c in CASES])
def test_contradicting_options_are_parser_errors(pkg, capsys, argv, message):
    from vitcpp_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(M + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and "vit: error:" in err and "Traceback" not in err, err
