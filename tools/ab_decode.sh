# A/B of the general decoder's routes on the 1 GiB bitmaps (tools/decode_ab.py): the two launches, then the one pass
cd $GRAFT_REPO_ROOT
DECODE_ROUTE=two timeout -k 10 120 python tools/decode_ab.py sparse dense || exit 1
timeout -k 10 120 python tools/decode_ab.py sparse dense || exit 1
