// mpc_fleet.h -- where a call's vehicle constants come from, on the host: the
// fleet objects of the C ABI and the launch that hands a kernel either one struct by value or a
// fleet's device table.  For the files whose kernels take a vehicle (mpc_linearise.hip,
// mpc_device.hip); the assembly takes none and stays clear of the models.
#pragma once
#include <type_traits>

#include "mpc_host.h"
#include "vehicle_model.h"

namespace mpcqp {

// A fleet: the B structs as given, each vehicle's constants (vehicle_constants, on the host, at
// creation) and their device table, uploaded by the first call that needs it.
template <class V, class KT>
struct Fleet {
    using Vehicle = V;
    using K = KT;
    int dev = 0;
    std::vector<V> veh;
    std::vector<KT> k;
    KT* d_k = nullptr;
};

}  // namespace mpcqp

struct mpcqp_fleet : mpcqp::Fleet<mpcqp_vehicle, mpcqp::VehicleK> {};
struct mpcqp_kin_fleet : mpcqp::Fleet<mpcqp_kin_vehicle, mpcqp_kin_vehicle> {};

namespace mpcqp {

// The constants' source of a call, V: a vehicle struct (one car for the batch, by value) or a fleet
// (its table, entry b for vehicle b).  Every host function that takes one is written once over V:
// source_check after its own argument checks and before any device call, then launch_from.
template <class V>
constexpr bool kIsFleet = std::is_same<V, mpcqp_fleet>::value || std::is_same<V, mpcqp_kin_fleet>::value;

// a fleet serves batches of its own size on its own device; a vehicle struct any
template <class V>
int source_check(const char* what, const V* veh, int64_t B, int device) {
    if constexpr (kIsFleet<V>) {
        if ((int64_t)veh->k.size() != B)
            return set_error(MPCQP_EINVAL, "%s: B = %lld is not the fleet's size %lld", what, (long long)B,
                             (long long)veh->k.size());
        if (veh->dev != device)
            return set_error(MPCQP_EINVAL, "%s: the fleet was created for device %d, the call is on device %d", what,
                             veh->dev, device);
    }
    return 0;
}

// the fleet's device table, uploaded here on first use
template <class F>
int fleet_table(const F* fleet, TableK<typename F::K>* out) {
    F& f = *const_cast<F*>(fleet);
    if (!f.d_k) {
        MHIPCHK(hipSetDevice(f.dev));
        if (int e = upload(f.k, &f.d_k)) return e;
    }
    out->k = f.d_k;
    return 0;
}

// launch(): `uniform` with the struct's constants, or `table` with the fleet's device table,
// first among the kernel's arguments
#define BOTH_FORMS(kernel, K) kernel<K>, kernel<TableK<K>>  // `uniform`, `table` of a kernel template over KS
template <class V, class KU, class KT, class... A>
int launch_from(const V* veh, int device, void* stream, long count, int block, KU uniform, KT table, A... args) {
    if constexpr (kIsFleet<V>) {
        TableK<typename V::K> t;
        if (int e = fleet_table(veh, &t)) return e;
        return launch(device, stream, count, block, table, t, args...);
    } else {
        return launch(device, stream, count, block, uniform, vehicle_constants(*veh), args...);
    }
}

}  // namespace mpcqp
