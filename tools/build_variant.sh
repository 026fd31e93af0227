#!/bin/bash
# Build an A/B variant of libwsg.so with extra -D flags into cppserver_amd/_build/var/<name>/.
#   tools/build_variant.sh NAME [-DFOO=1 ...]
#   $KSRC: other sources in place of wsg_decode.hip wsg_encode.hip wsg_fanout.hip wsg_lane_device.hip wsg_misc.hip,
#   e.g. the one wsg_kernels.hip of a revision from before they left it (a source finds the headers beside it first,
#   so an older one builds inside an export of its own csrc/);
#   $CSRC: other C-ABI sources in place of wsg_capi.cpp wsg_lane.cpp wsg_capi_device.cpp wsg_capi_host.cpp, e.g. an
#   older wsg_capi.hip;
#   $PSRC: the pipeline kernel sources, "" for a wsg_kernels.hip from before they left it
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/cppserver_amd/_build/var/$name
mkdir -p "$out"
cd "$out"
H=/opt/rocm/bin/hipcc
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$root/include $*"
csrc=$root/cppserver_amd/csrc
kobjs=
for k in ${KSRC:-$csrc/wsg_decode.hip $csrc/wsg_encode.hip $csrc/wsg_fanout.hip $csrc/wsg_lane_device.hip $csrc/wsg_misc.hip}; do
    o=k_$(basename "$k" .hip).o
    $H $F -I$csrc -c "$k" -o "$o"
    kobjs="$kobjs $o"
done
pobjs=
for p in ${PSRC-$csrc/wsg_messages.hip $csrc/wsg_frames.hip $csrc/wsg_utf8.hip $csrc/wsg_proto.hip $csrc/wsg_assembly.hip $csrc/wsg_upgrade.hip $csrc/wsg_carry.hip $csrc/wsg_relay.hip}; do
    o=p_$(basename "$p" .hip).o
    $H $F -I$csrc -c "$p" -o "$o"
    pobjs="$pobjs $o"
done
cobjs=
for c in ${CSRC-$csrc/wsg_capi.cpp $csrc/wsg_lane.cpp $csrc/wsg_capi_device.cpp $csrc/wsg_capi_host.cpp}; do
    o=c_$(basename "${c%.*}").o
    case $c in *.hip) $H $F -I$csrc -c "$c" -o "$o" ;; *) $H -O3 -std=c++17 -fPIC -I$root/include $* -I$csrc -c "$c" -o "$o" ;; esac
    cobjs="$cobjs $o"
done
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/ws.cpp -o w.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/ws_api.cpp -o a.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/ws_batch.cpp -o b.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/http.cpp -o h.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/tls.cpp -o t.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/wss.cpp -o s.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/wsg_mgpu.cpp -o m.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/wsg_proto_host.cpp -o j.o
$H -O3 -std=c++17 -fPIC -I$root/include -c $root/cppserver_amd/csrc/wsg_upgrade_host.cpp -o u.o
$H --offload-arch=gfx950 -shared -o libwsg.so $kobjs $pobjs $cobjs w.o a.o b.o h.o t.o s.o m.o j.o u.o -lssl -lcrypto -ldl -L/opt/rocm/lib -lrocprofiler-sdk-roctx
echo "$out/libwsg.so"
