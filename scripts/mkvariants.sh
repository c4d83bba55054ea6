#!/bin/bash
# Build variants of libtlsan_hip.so for an A/B (where the tree is built; hipcc cross-compiles):
#   scripts/mkvariants.sh stamps:"-DTLSAN_STAMPS=1" fp@tlsan_attn_d64,tlsan_attn_d128:"-ffp-contract=off" rev:HEAD~1 ...
#     name:"flags"              extra compiler flags on every unit (TLSAN_HIPCC_EXTRA)
#     name@unit1,unit2:"flags"  the named units compiled with these flags in place of their own (TLSAN_SOURCE_FLAGS)
#     rev:<commit>              that commit's library, built in a temporary worktree -> ab_run/rev_<commit>.so
# -> ab_run/<name>.so (git-ignored; emptied when the experiment is over).  `base`, the tree as it stands, is always built,
# last, so the tree's own library is left as the default build.  Run them on ONE GPU machine with scripts/ab.py --libs.
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
mkdir -p ab_run
O=tlsan_amd/csrc/build
tmp=

build() {  # tree: builds its library quietly
  (cd "$1" && python -c "from tlsan_amd import build; build.build()" > /dev/null)
}
forget() {  # units (none: all): their objects, which do not know the flags they were compiled with
  if [ $# -eq 0 ]; then rm -f $O/*.o; else for u in "$@"; do rm -f "$O/${u%.hip}.o"; done; fi
}
cleanup() {
  if [ -n "$tmp" ]; then git worktree remove --force "$tmp/tree" 2> /dev/null || true; rmdir "$tmp" 2> /dev/null || true; git worktree prune; fi
}
trap cleanup EXIT

for spec in "$@"; do
  name="${spec%%:*}"; arg="${spec#*:}"
  if [ "$name" = "rev" ]; then
    tmp=$(mktemp -d)
    git worktree add -q --detach "$tmp/tree" "$arg"
    build "$tmp/tree"
    out="ab_run/rev_$(echo "$arg" | tr -c 'A-Za-z0-9._\n' '_').so"
    cp "$tmp/tree/tlsan_amd/libtlsan_hip.so" "$out"
    cleanup; tmp=
    echo "built $out  [git $arg]"
  elif [[ "$name" == *@* ]]; then
    IFS=, read -r -a units <<< "${name#*@}"; name="${name%%@*}"
    js=$(python3 -c "import json, sys; print(json.dumps({u.replace('.hip', '') + '.hip': sys.argv[1].split() for u in sys.argv[2:]}))" "$arg" "${units[@]}")
    forget "${units[@]}"
    TLSAN_SOURCE_FLAGS="$js" build .
    forget "${units[@]}"
    cp tlsan_amd/libtlsan_hip.so "ab_run/$name.so"
    echo "built ab_run/$name.so  [${units[*]}: $arg]"
  else
    forget
    TLSAN_HIPCC_EXTRA="$arg" build .
    [ -z "$arg" ] || forget
    cp tlsan_amd/libtlsan_hip.so "ab_run/$name.so"
    echo "built ab_run/$name.so  [$arg]"
  fi
done
build .
cp tlsan_amd/libtlsan_hip.so ab_run/base.so
echo "built ab_run/base.so  [the tree]"
