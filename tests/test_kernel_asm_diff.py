"""tools/kernel_asm_diff.py: the comparison that a deletion or refactor of device code is accepted by -- every function present in both
assembly files has the same instructions, whatever was removed in front of it (no GPU needed; no reference counterpart: a build tool)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_asm_diff as K      # noqa: E402

OLD = '''
	.text
_Z4deadv:                               ; @_Z4deadv
.Lfunc_begin0:
; %bb.0:
	s_endpgm
.Lfunc_end0:
	.size	_Z4deadv, .Lfunc_end0-_Z4deadv
                                        ; -- End function
_Z4keepPf:                              ; @_Z4keepPf
.Lfunc_begin1:
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_cbranch_scc1 .LBB1_2
; %bb.1:
	v_add_f32_e32 v0, 1.0, v0               ; function 1
.LBB1_2:
.Ltmp1:
	s_endpgm
.Lfunc_end1:
	.size	_Z4keepPf, .Lfunc_end1-_Z4keepPf
__hip_cuid_0123:
	.byte	0
'''
# the same file without the first function: the survivor's index moves from 1 to 0
NEW = OLD[:OLD.index('_Z4deadv:')] + OLD[OLD.index('_Z4keepPf:'):].replace('func_begin1', 'func_begin0').replace('func_end1', 'func_end0') \
    .replace('.LBB1_', '.LBB0_').replace('.Ltmp1', '.Ltmp0').replace('; function 1', '; function 0')
CHANGED = NEW.replace('v_add_f32_e32 v0, 1.0, v0', 'v_add_f32_e32 v0, 2.0, v0')


def test_identical_bodies_under_shifted_function_indices_pass_and_the_removed_function_is_reported(tmp_path, capsys):
    assert sorted(K.functions(OLD)) == ['_Z4deadv', '_Z4keepPf'] and len(K.functions(OLD)['_Z4keepPf']) == 7
    assert K.compare(OLD, NEW) == (['_Z4deadv'], [], [])
    a, b = tmp_path / 'old.s', tmp_path / 'new.s'
    a.write_text(OLD); b.write_text(NEW)
    assert K.main(['', str(a), str(b)]) == 0
    assert 'removed: _Z4deadv' in capsys.readouterr().out


def test_one_changed_instruction_fails(tmp_path, capsys):
    assert K.compare(OLD, CHANGED) == (['_Z4deadv'], [], ['_Z4keepPf'])
    a, b = tmp_path / 'old.s', tmp_path / 'new.s'
    a.write_text(OLD); b.write_text(CHANGED)
    assert K.main(['', str(a), str(b)]) == 1
    assert 'DIFFERS: _Z4keepPf' in capsys.readouterr().out


def test_an_added_function_fails():
    assert K.compare(NEW, OLD) == ([], ['_Z4deadv'], [])
    assert K.compare(OLD, OLD) == ([], [], [])
