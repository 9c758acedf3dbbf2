"""Function-by-function comparison of two device assembly files (the Makefile's build/isa/%.s rule: hipcc --cuda-device-only -S).
The acceptance check of a deletion / refactor that must leave the surviving device code alone: every function present in both files has the same
instructions.  Comments (after `;`) are dropped and the per-file function index in local labels (.LBB<n>_, .Ltmp<n>, .Lfunc_*<n>) is normalised, so
that removing a function in front of another one does not count as a change of the latter.
usage: python tools/kernel_asm_diff.py old.s new.s     (exit status 1 when a common function differs or a function was added)"""
import re
import sys

GLOBAL = re.compile(r'^([A-Za-z_$][\w$.]*):')
LOCAL = re.compile(r'\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+')


def functions(text):
    """{name: [normalised body lines]} -- a function runs from its label line to its .Lfunc_end label."""
    out, name = {}, None
    for raw in text.splitlines():
        line = raw.split(';', 1)[0].rstrip()
        m = GLOBAL.match(line)
        if m:                                       # a global label (local ones start with a dot): a function starts (a data label never reaches a .Lfunc_end and is dropped)
            name, body = m.group(1), []
        elif name is None:
            continue
        elif line.startswith('.Lfunc_end'):
            out[name], name = body, None
        elif line.strip():
            body.append(LOCAL.sub(r'.\1#', line))
    return out


def compare(old_text, new_text):
    """-> (removed, added, differing) lists of function names"""
    old, new = functions(old_text), functions(new_text)
    return (sorted(set(old) - set(new)), sorted(set(new) - set(old)), sorted(n for n in set(old) & set(new) if old[n] != new[n]))


def main(argv):
    old_text, new_text = open(argv[1]).read(), open(argv[2]).read()
    removed, added, differing = compare(old_text, new_text)
    print(f'{argv[1]} -> {argv[2]}: {len(functions(old_text))} -> {len(functions(new_text))} functions; '
          f'{len(removed)} removed, {len(added)} added, {len(differing)} differing')
    for kind, names in (('removed', removed), ('added', added), ('DIFFERS', differing)):
        for n in names:
            print(f'  {kind}: {n}')
    return 1 if added or differing else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
