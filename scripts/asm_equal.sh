#!/bin/bash
# Usage: scripts/asm_equal.sh <git-rev> [file.hip ...]
# Proof for a kernel refactor that must not change one emitted instruction: compiles every source of the Makefile's SRCS
# (or only the files named) from <git-rev> and from the working tree to assembly, device side and host side, with exactly
# the command line the Makefile uses for that file, and diffs the two.  hipcc names a few symbols after a hash of the source
# text (__hip_cuid_<hash>; on the host side also __hip_fatbin_<hash> and __hip_gpubin_handle_<hash>): each file's own hash,
# read from its __hip_cuid_ symbol, is replaced by the word CUID before the diff; anything else that differs is a difference.
# Prints one line per file, with a verdict for each side, and exits non-zero when any file differs on either side.  Needs no GPU.  JOBS (default 8) compiles run at once.
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 <git-rev> [file.hip ...]" >&2; exit 2; }
REV=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=torch_em_amd/csrc
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/old" "$TMP/asm"
git -C "$ROOT" archive "$REV" $CSRC include | tar -x -C "$TMP/old"

# the Makefile's own compile lines, one per source: "<hipcc> <flags> -c <file>.hip -o <object>"
make -n -B -C "$ROOT/$CSRC" all | grep -- ' -c ' > "$TMP/lines"
if [ $# -gt 0 ]; then
  for f in "$@"; do grep -- " -c $f " "$TMP/lines" || { echo "$f is not in SRCS" >&2; exit 2; }; done > "$TMP/sel"
  mv "$TMP/sel" "$TMP/lines"
fi

while read -r line; do
  src=$(sed 's/.* -c \([^ ]*\) -o .*/\1/' <<< "$line")
  cmd=${line%% -c *}
  for side in old new; do
    dir=$ROOT/$CSRC; [ $side = old ] && dir=$TMP/old/$CSRC
    for mode in device host; do
      echo "cd $dir && $cmd -Wno-unused-command-line-argument --cuda-$mode-only -S $src -o $TMP/asm/${src%.hip}.$side.$mode.s"
    done
  done
done < "$TMP/lines" > "$TMP/jobs"
xargs -d '\n' -P "${JOBS:-8}" -n 1 sh -c < "$TMP/jobs"

# the file with its source-text hash replaced (a file without the symbol passes through unchanged)
norm() {
  local h; h=$(grep -o '__hip_cuid_[0-9a-f]*' "$1" | head -n 1 | sed 's/__hip_cuid_//' || true)
  if [ -n "$h" ]; then sed "s/$h/CUID/g" "$1" > "$2"; else cp "$1" "$2"; fi
}
rc=0; ndev=0; nhost=0
for src in $(sed 's/.* -c \([^ ]*\) -o .*/\1/' "$TMP/lines"); do
  for mode in device host; do
    a=$TMP/asm/${src%.hip}.old.$mode.s; b=$TMP/asm/${src%.hip}.new.$mode.s
    norm "$a" "$TMP/a.s"; norm "$b" "$TMP/b.s"
    eval "v_$mode=same"
    if ! diff "$TMP/a.s" "$TMP/b.s" > "$TMP/d"; then
      eval "v_$mode=DIFFERENT"; rc=1
      [ $mode = device ] && ndev=$((ndev + 1)) || nhost=$((nhost + 1))
      echo "--- $src ($mode): first differing lines" >&2; head -20 "$TMP/d" >&2
    fi
  done
  printf '%-22s (device) %-9s (host) %-9s  (device %d lines, host %d lines)\n' "$src" $v_device $v_host \
    "$(wc -l < "$TMP/asm/${src%.hip}.new.device.s")" "$(wc -l < "$TMP/asm/${src%.hip}.new.host.s")"
done
echo "files that differ: (device) $ndev, (host) $nhost"
exit $rc
