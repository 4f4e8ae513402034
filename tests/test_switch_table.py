"""The `CGG_*` environment surface is the table in README.md ("Environment switches"), no more and no less: every name the package,
tools/, bench.py or tests/ read from the environment has a row that states why it exists, and every row is still read somewhere.
A new switch therefore cannot be added without a stated reason, and a retired one cannot linger in the table."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, 'betrayed-by-captions_amd')

# a literal CGG_ name as the first argument of environ.get / the key of environ[...] (Python) or of getenv (csrc/)
READ = re.compile(r'''(?:environ\s*(?:\.get\s*\(|\[)|getenv\s*\()\s*['"](CGG_[A-Z0-9_]+)['"]''')
ROW = re.compile(r'^\|\s*`(CGG_[A-Z0-9_]+)`\s*\|')
REASONS = ('escape', 'fallback handle', 'test reference', 'parameter')


def _sources():
    yield os.path.join(ROOT, 'bench.py')
    for top in (PACKAGE, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')):
        for d, _, files in os.walk(top):
            for f in files:
                if f.endswith(('.py', '.hip', '.h', '.sh')):
                    yield os.path.join(d, f)


def _names_read():
    found = {}
    for path in _sources():
        with open(path, encoding='utf-8') as fh:
            for name in READ.findall(fh.read()):
                found.setdefault(name, os.path.relpath(path, ROOT))
    return found


def _table():
    rows = {}
    with open(os.path.join(ROOT, 'README.md'), encoding='utf-8') as fh:
        for line in fh:
            m = ROW.match(line)
            if m:
                assert m.group(1) not in rows, f'{m.group(1)} has two rows'
                rows[m.group(1)] = [c.strip() for c in line.strip().strip('|').split('|')]
    return rows


def test_every_switch_read_has_a_readme_row_and_every_row_is_read():
    read, rows = _names_read(), _table()
    assert len(read) >= 20 and len(rows) >= 20, 'the scan or the table parse found (almost) nothing'
    missing = {n: read[n] for n in sorted(set(read) - set(rows))}
    stale = sorted(set(rows) - set(read))
    assert not missing, f'read from the environment without a row in the README table: {missing}'
    assert not stale, f'rows of the README table that nothing reads any more: {stale}'


def test_every_row_states_default_effect_and_reason():
    for name, cells in _table().items():
        assert len(cells) == 4 and all(cells), (name, cells)
        assert cells[3] in REASONS, (name, cells[3])


def test_the_switch_tests_only_flip_names_of_the_table():
    """a row of tests/test_env_switches_gpu.py that names a retired switch would silently re-test the default path"""
    rows = _table()
    with open(os.path.join(ROOT, 'tests', 'test_env_switches_gpu.py'), encoding='utf-8') as fh:
        flipped = set(re.findall(r"'(CGG_[A-Z0-9_]+)=", fh.read()))
    assert len(flipped) >= 15 and flipped <= set(rows), sorted(flipped - set(rows))
